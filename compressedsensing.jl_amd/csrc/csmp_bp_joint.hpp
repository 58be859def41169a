// csmp_bp_joint.hpp -- gfx950 kernels of csmp_bp_joint (host/bp_joint.hpp): row-sparse basis pursuit (the l2,1 "MMV" programme)
//     min sum_j w_j ||X[j, :]||_2   subject to   A X = B
// for columns of B that share ONE support -- csmp_bp's ADMM (csmp_bp.hpp) with matrices in place of vectors and the shrinkage on whole
// rows.  Z, U: N x nsig; P = A Z, Q = A U, E, V, Y, G Y: M x nsig; t_j = w_j / rho.  One iteration:
//     E = P - Q - B;   V = R^-T E,  Y = R^-1 V,  G Y   (k_bp_gemm, chunks of up to eight columns);   C = A'Y (csmp_somp's passes)
//     T = Z - C;   n_j = sqrt(sum_l T[j,l]^2);   Z+[j,:] = 0 where !(n_j > t_j), else (1 - t_j / n_j) T[j,:];   U+ = T - Z+
//     R = B - A Z+  (k_jista_axpy / k_jista_resum over the ONE list of Z+);   P+ = B - R;   Q+ = P - G Y - P+
//   k_jbp_start    the start from Z = U = 0 for every column: P = Q = 0, E = -B
//   k_jbp_update   the row-wise step over the N atoms, the ONE list of the non-zero rows of Z+ (k_jista_update's layout: k_jista_axpy
//                  consumes it unchanged) and the segments' partials of ||U+ - U||_F^2 and ||Z+ - Z||_F^2 (k_bp_update's layout:
//                  k_bp_fold adds them unchanged)
//   k_jbp_pq       bp_pq_body for every column
//   k_jbp_norm2    k_norm2 for every column
//
// Determinism: n_j is added by fma in column order; the list is in ascending index order; a thread adds its atoms' shares of the two
// squared norms in atom order and per atom in column order, block_sum256 adds the threads, k_bp_fold the segments.  No atomics, no
// workgroup waits for another: the same bits on every run and for every cut of the columns into chunks.
#pragma once
#include "csmp_bp.hpp"
#include "csmp_ista_joint.hpp"

namespace csmp {

// P = Q = 0, E = -B (k_bp_start) for every column: column l owns the wgs = ceil(M / 256) workgroups from l * wgs, as in k_somp_init
__global__ __launch_bounds__(256) void k_jbp_start(const double* __restrict__ Bd, int64_t ldr, int M, int nsig, int wgs, double* __restrict__ P,
                                                   double* __restrict__ Q, double* __restrict__ E) {
    const int l = (int)(blockIdx.x / (unsigned)wgs), i = (int)(blockIdx.x % (unsigned)wgs) * 256 + (int)threadIdx.x;
    if (l >= nsig || i >= M) return;
    const int64_t at = (int64_t)l * ldr + i;
    P[at] = 0.0;
    Q[at] = 0.0;
    E[at] = -Bd[at];
}

// P+, Q+ and the next E of every column: bp_pq_body on column l's M-vectors (all from l * ldr), the grid as k_jbp_start's
__global__ __launch_bounds__(256) void k_jbp_pq(const double* __restrict__ Bd, const double* __restrict__ R, const double* __restrict__ GY,
                                                int64_t ldr, int M, int nsig, int wgs, double* __restrict__ P, double* __restrict__ Q,
                                                double* __restrict__ E) {
    const int l = (int)(blockIdx.x / (unsigned)wgs);
    if (l >= nsig) return;
    const int64_t at = (int64_t)l * ldr;
    bp_pq_body((int)(blockIdx.x % (unsigned)wgs), Bd + at, R + at, GY + at, M, P + at, Q + at, E + at);
}

// The step for every row.  One workgroup per segment of atoms, one thread per atom j (k_jista_update's segmentation), columns
// l = 0, 1, ... in turn: for each l the threads of a wave read consecutive atoms of c_l, z_l and u_l.  The loop over the columns runs
// TWICE -- once for n_j, once for the scaled row and U -- so a thread holds a handful of values whatever nsig is (the second loop's
// reads of c and z hit the cache lines the first brought in).  A row is listed when one or more entries of Z+ are non-zero; the values of
// list entry e are lval[e * nsig + l].  rpart[s] = the segment's share of ||U+ - U||_F^2, rpart[kIstaMaxSegs + s] of ||Z+ - Z||_F^2.
// C: column l from l * ldc; Z, U: column l from l * ldx.
__global__ __launch_bounds__(kIstaThreads) void k_jbp_update(const double* __restrict__ C, int64_t ldc, const double* __restrict__ w, int64_t nw,
                                                             double rho, double* __restrict__ Z, double* __restrict__ U, int64_t ldx, int nsig,
                                                             int64_t N, int64_t seg_len, int* __restrict__ lidx, double* __restrict__ lval,
                                                             int* __restrict__ seg_cnt, double* __restrict__ rpart) {
    __shared__ int wcnt[kIstaThreads / kWave];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned seg = blockIdx.x;
    const int64_t j0 = (int64_t)seg * seg_len, j1 = j0 + seg_len < N ? j0 + seg_len : N;
    const double w0 = w[0];
    double sp = 0.0, sd = 0.0;
    int64_t base = j0;
    for (int64_t jt = j0; jt < j1; jt += kIstaThreads) {
        const int64_t j = jt + tid;
        bool nz = false;
        if (j < j1) {
            const double tj = (nw == 1 ? w0 : w[j]) / rho;
            double n2 = 0.0;
#pragma unroll 4
            for (int l = 0; l < nsig; ++l) {
                const double t = Z[(int64_t)l * ldx + j] - C[(int64_t)l * ldc + j];
                n2 = fma(t, t, n2);
            }
            const double nj = sqrt(n2);
            const bool live = nj > tj;
            const double sc = live ? 1.0 - tj / nj : 0.0;
#pragma unroll 4
            for (int l = 0; l < nsig; ++l) {
                const double zo = Z[(int64_t)l * ldx + j], uo = U[(int64_t)l * ldx + j];
                const double t = zo - C[(int64_t)l * ldc + j];
                const double zn = live ? sc * t : 0.0;
                const double un = t - zn;
                Z[(int64_t)l * ldx + j] = zn;
                U[(int64_t)l * ldx + j] = un;
                const double du = un - uo, dz = zn - zo;
                sp = fma(du, du, sp);
                sd = fma(dz, dz, sd);
                nz = nz || zn != 0.0;
            }
        }
        const unsigned long long mask = __ballot(nz);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < kIstaThreads / kWave; ++q) {
            before += q < wave ? wcnt[q] : 0;
            all += wcnt[q];
        }
        if (nz) {
            const int64_t p = base + before + __popcll(mask & ((1ull << lane) - 1ull));
            lidx[p] = (int)j;
            double* __restrict__ lv = lval + p * nsig;
#pragma unroll 4
            for (int l = 0; l < nsig; ++l) lv[l] = Z[(int64_t)l * ldx + j];  // (this thread's own stores of above)
        }
        base += all;
        __syncthreads();
    }
    sp = block_sum256(sp, red);
    sd = block_sum256(sd, red);
    if (tid == 0) {
        seg_cnt[seg] = (int)(base - j0);
        rpart[seg] = sp;
        rpart[kIstaMaxSegs + seg] = sd;
    }
}

// out[l] = ||r_l||^2 by workgroup l, with k_norm2's operations in k_norm2's order: what csmp_bp reports for the same residual
__global__ __launch_bounds__(256) void k_jbp_norm2(const double* __restrict__ R, int64_t ldr, int M, double* __restrict__ out) {
    __shared__ double s[256];
    const double* __restrict__ r = R + (int64_t)blockIdx.x * ldr;
    double acc = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) acc = fma(r[i], r[i], acc);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if ((int)threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

}  // namespace csmp
