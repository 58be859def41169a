// csmp_ista_joint.hpp -- gfx950 kernels of csmp_ista_joint (host/ista_joint.hpp): ISTA / FISTA on the row-sparse (l2,1, "MMV") objective
//     ||B - A X||_F^2 + sum_j w_j ||X[j, :]||_2
// for columns of B that share ONE support -- the convex counterpart of csmp_somp.  One iteration, alpha = stepsize, t_j = w_j alpha:
//     R = B - A Y;   C = A'R (the shared pass of csmp_somp, unchanged);   U = Y + 2 alpha C;   n_j = sqrt(sum_l U[j,l]^2)
//     X+[j,:] = 0 where !(n_j > t_j), else (1 - t_j / n_j) U[j,:];        Y+ = X+ + beta (X+ - X)      (beta = 0: ISTA, Y = X)
//   k_jista_update   the row-wise step over the N atoms, and the ONE list of the non-zero rows of the next Y
//   k_jista_axpy     R's subtrahend  sum_j a_j Y[j, l]  over that list for a chunk of up to eight columns l: every live column of A is
//                    read ONCE for the chunk (csmp_ista_batch reads it once per signal), one partial M-vector per workgroup and column
//   k_jista_resum    r_l = b_l - (the partials, added in workgroup order)
//   k_jista_norm2    ||r_l||^2 of every column
//
// The list is csmp_ista.hpp's: SEGMENTS of atoms, workgroup s of k_jista_update owns the atoms [s seg_len, (s + 1) seg_len), writes the
// indices of their non-zero rows in ascending order to lidx from entry s seg_len on and their number to seg_cnt[s]; the readers scan
// seg_cnt themselves (ista_seg_scan).  The VALUES of entry e are the nsig numbers lval[e * nsig + l], l = 0 .. nsig): a row of Y, so the
// chunk [c0, c0 + NS) of k_jista_axpy reads the NS coefficients of a column of A as one contiguous piece.
//
// Determinism: n_j is added in column order; the list is in ascending index order; the split of the list over the workgroups is
// ista_parts(n, P) with csmp_ista's P, which depends on the list's length only; a workgroup adds a column's terms by fma in list
// order, k_jista_resum adds the partials in k_ista_resum's order.  So the sums of column l depend neither on the chunk it is in nor on
// the chunk's width, and where the joint list equals a signal's own list they are k_ista_axpy's bit for bit.  No atomics.
#pragma once
#include "csmp_ista.hpp"

namespace csmp {

constexpr int kJistaChunk = 8;  // columns a k_jista_axpy launch serves at the most

// 16-byte loads per lane and column of A, and columns in flight per wave: NS * L * VEC Float64 accumulators per lane, 32 at the most
// (64 VGPRs; 16 for one or two columns, where four loads per column and two sets made the compiler hold 256 VGPRs and 14 AGPRs), and a
// ring of NB * L = 8 .. 16 loads (32 .. 64 VGPRs)
template <typename TA, int NS>
struct JistaShape {
    static constexpr int want = (NS <= 2 ? 16 : 32) / (NS * Vec<TA>::n);
    static constexpr int L = want > kIstaL ? kIstaL : (want < 1 ? 1 : want);
    static constexpr int NB = L >= 4 ? 4 : 8;
};

// The step for every row.  One thread per atom j, columns l = 0, 1, ... in turn (for each l the threads of a wave read consecutive
// atoms of c_l and y_l).  ISTA_INIT: X = Y as it stands (the warm start), no step.  ISTA_LIST_X: the list is that of X+ instead of Y+
// (the last iteration: the residual of the RESULT follows).  A row is listed when one or more of its entries is non-zero.
// C: column l from l * ldc; X, Y: column l from l * ldx.
__global__ __launch_bounds__(kIstaThreads) void k_jista_update(const double* __restrict__ C, int64_t ldc, const double* __restrict__ w,
                                                               int64_t nw, double* __restrict__ X, double* __restrict__ Y, int64_t ldx,
                                                               int nsig, int64_t N, int64_t seg_len, double alpha, double beta, int flags,
                                                               int* __restrict__ lidx, double* __restrict__ lval, int* __restrict__ seg_cnt) {
    __shared__ int wcnt[kIstaThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned seg = blockIdx.x;
    const int64_t j0 = (int64_t)seg * seg_len, j1 = j0 + seg_len < N ? j0 + seg_len : N;
    const double w0 = w[0];
    const double* __restrict__ src = (flags & ISTA_LIST_X) ? X : Y;  // (what the list holds)
    int64_t base = j0;
    for (int64_t jt = j0; jt < j1; jt += kIstaThreads) {
        const int64_t j = jt + tid;
        bool nz = false;
        if (j < j1) {
            if (flags & ISTA_INIT) {
#pragma unroll 4
                for (int l = 0; l < nsig; ++l) {
                    const double yv = Y[(int64_t)l * ldx + j];
                    X[(int64_t)l * ldx + j] = yv;
                    nz = nz || yv != 0.0;
                }
            } else {
                const double tj = (nw == 1 ? w0 : w[j]) * alpha;
                double n2 = 0.0;
#pragma unroll 4
                for (int l = 0; l < nsig; ++l) {
                    const double u = Y[(int64_t)l * ldx + j] + 2.0 * alpha * C[(int64_t)l * ldc + j];
                    n2 = fma(u, u, n2);
                }
                const double nj = sqrt(n2);
                const bool live = nj > tj;
                const double sc = live ? 1.0 - tj / nj : 0.0;
#pragma unroll 4
                for (int l = 0; l < nsig; ++l) {
                    const double yv = Y[(int64_t)l * ldx + j];
                    const double u = yv + 2.0 * alpha * C[(int64_t)l * ldc + j];
                    const double xn = live ? sc * u : 0.0;
                    const double yn = (flags & ISTA_ACCEL) ? xn + beta * (xn - X[(int64_t)l * ldx + j]) : xn;
                    X[(int64_t)l * ldx + j] = xn;
                    Y[(int64_t)l * ldx + j] = yn;
                    nz = nz || ((flags & ISTA_LIST_X) ? xn : yn) != 0.0;
                }
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
            for (int l = 0; l < nsig; ++l) lv[l] = src[(int64_t)l * ldx + j];  // (this thread's own stores of above)
        }
        base += all;
        __syncthreads();
    }
    if (tid == 0) seg_cnt[seg] = (int)(base - j0);
}

// part[(l * P + p) * Mv + row] = sum over workgroup p's share of the list of  Y[idx_t, c0 + l] * A[row, idx_t]  for the columns
// l = 0 .. size) of the chunk that starts at column c0, size <= NS, and the row block blockIdx.y: kIstaThreads / 64 waves x 64 lanes x
// L vectors of 16 bytes.  ista_axpy_body with NS accumulator sets: the list's tiles staged in the LDS (the indices, and the NS values of
// every entry side by side), a ring of NB columns of 16-byte non-temporal loads per wave, every loaded piece of a_j feeding the NS
// sets.  Grid (P, row blocks): P is csmp_ista's (ista_parts_max), the workgroups beyond ista_parts(n, P) leave at once.
// Ragged columns: a lane past the column's end re-reads the column's last vector and its sums are not stored.  Set l >= size of a
// chunk narrower than NS repeats set size - 1 and is not stored.
template <typename TA, int NS>
__global__ __launch_bounds__(kIstaThreads) void k_jista_axpy(const TA* __restrict__ A, int64_t ld, int Mv, const int* __restrict__ seg_cnt,
                                                             int nseg, int64_t seg_len, const int* __restrict__ lidx,
                                                             const double* __restrict__ lval, int nsig, int c0, int size,
                                                             double* __restrict__ part, unsigned* __restrict__ nnz_out) {
    using VT = typename Vec<TA>::type;
    constexpr int VEC = Vec<TA>::n, L = JistaShape<TA, NS>::L, NB = JistaShape<TA, NS>::NB;
    static_assert(kIstaTile % NB == 0 && NS * L * VEC <= 32, "the ring divides a tile; the accumulators fit the register budget");
    __shared__ unsigned off[kIstaMaxSegs + 1];
    __shared__ unsigned ws[kIstaThreads];
    __shared__ int tidx[kIstaTile];
    __shared__ double tval[kIstaTile * NS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = blockIdx.x, P = gridDim.x;
    const unsigned n = ista_seg_scan(seg_cnt, nseg, off, ws);
    if (p == 0 && blockIdx.y == 0 && tid == 0) *nnz_out = n;
    const int Pa = ista_parts(n, P);
    if (p >= Pa) return;
    const unsigned lo = (unsigned)((uint64_t)p * n / Pa), hi = (unsigned)((uint64_t)(p + 1) * n / Pa);
    const int nvec = Mv / VEC;
    const int v0 = ((int)blockIdx.y * (kIstaThreads / kWave) + wave) * (kWave * L);  // the wave's first vector of a column
    const bool active = v0 < nvec;
    int vq[L];
#pragma unroll
    for (int q = 0; q < L; ++q) vq[q] = min(v0 + q * kWave + lane, nvec - 1);
    VT buf[NB][L];
    double acc[NS][L * VEC];
#pragma unroll
    for (int l = 0; l < NS; ++l)
#pragma unroll
        for (int q = 0; q < L * VEC; ++q) acc[l][q] = 0.0;
    auto issue = [&](VT(&b)[L], int i) {
        const int j = __builtin_amdgcn_readfirstlane(tidx[i]);
        const VT* pc = reinterpret_cast<const VT*>(A + (int64_t)j * ld);
#pragma unroll
        for (int q = 0; q < L; ++q) b[q] = __builtin_nontemporal_load(pc + vq[q]);
    };
    auto consume = [&](const VT(&b)[L], int i) {
        double yv[NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) yv[l] = tval[i * NS + l];
#pragma unroll
        for (int q = 0; q < L; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const double a = (double)b[q][e];
#pragma unroll
                for (int l = 0; l < NS; ++l) acc[l][q * VEC + e] = fma(a, yv[l], acc[l][q * VEC + e]);
            }
    };
    for (unsigned t0 = lo; t0 < hi; t0 += kIstaTile) {
        const int nt = (int)min((unsigned)kIstaTile, hi - t0);
        __syncthreads();  // (the previous tile has been consumed by every wave)
        if (tid < nt) {
            const unsigned pos = t0 + tid;
            int a = 0, z = nseg;  // the segment with off[a] <= pos < off[a + 1]
            while (z - a > 1) {
                const int mid = (a + z) >> 1;
                if (off[mid] <= pos) a = mid; else z = mid;
            }
            const int64_t e = (int64_t)a * seg_len + (pos - off[a]);
            tidx[tid] = lidx[e];
            const double* __restrict__ lv = lval + e * nsig + c0;
#pragma unroll
            for (int l = 0; l < NS; ++l) tval[tid * NS + l] = lv[min(l, size - 1)];
        }
        __syncthreads();
        if (!active) continue;
        // the ring: NB columns in flight, a consumed buffer is refilled at once with the column NB ahead
#pragma unroll
        for (int d = 0; d < NB; ++d) issue(buf[d], min(d, nt - 1));
        int i = 0;
        for (int g = 0; g + 1 < nt / NB; ++g, i += NB) {
#pragma unroll
            for (int d = 0; d < NB; ++d) {
                consume(buf[d], i + d);
                issue(buf[d], i + NB + d);
            }
        }
#pragma unroll
        for (int d = 0; d < NB; ++d) {  // the last NB .. 2 NB - 1 columns of the tile (or all of them, when there are fewer)
            if (i + d < nt) {
                consume(buf[d], i + d);
                if (i + NB + d < nt) issue(buf[d], i + NB + d);
            }
        }
#pragma unroll
        for (int d = 0; d < NB; ++d)
            if (i + NB + d < nt) consume(buf[d], i + NB + d);
    }
    if (!active) return;
#pragma unroll
    for (int l = 0; l < NS; ++l) {
        if (l >= size) break;
        double* out = part + ((int64_t)l * P + p) * Mv;
#pragma unroll
        for (int q = 0; q < L; ++q) {
            const int v = v0 + q * kWave + lane;
            if (v < nvec) {
#pragma unroll
                for (int e = 0; e < VEC; e += 2) {
                    f64x2 s2;
                    s2.x = acc[l][q * VEC + e];
                    s2.y = acc[l][q * VEC + e + 1];
                    *reinterpret_cast<f64x2*>(out + (int64_t)v * VEC + e) = s2;
                }
            }
        }
    }
}

// r_l = b_l - (the first ista_parts(n, P) partials of column l, in workgroup order): ista_resum_body for the column blockIdx.y of the
// chunk -- its partials from l * P * Mv, b and r: column c from c * ldr, c = c0 + l.
__global__ __launch_bounds__(kIstaThreads) void k_jista_resum(const double* __restrict__ part, int Mv, int M, const unsigned* __restrict__ nnz,
                                                              int P, const double* __restrict__ Bd, double* __restrict__ R, int64_t ldr, int c0) {
    const int64_t l = blockIdx.y, c = c0 + l;
    ista_resum_body(part + l * P * Mv, Mv, M, nnz, P, Bd + c * ldr, R + c * ldr);
}

// out[l] = ||r_l||^2 by workgroup l: thread t adds the rows t, t + 256, ... in turn, block_sum256 over the threads
__global__ __launch_bounds__(256) void k_jista_norm2(const double* __restrict__ R, int64_t ldr, int M, double* __restrict__ out) {
    __shared__ double sc[4];
    const double* __restrict__ r = R + (int64_t)blockIdx.x * ldr;
    double d = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) d = fma(r[i], r[i], d);
    d = block_sum256(d, sc);
    if (threadIdx.x == 0) out[blockIdx.x] = d;
}

}  // namespace csmp
