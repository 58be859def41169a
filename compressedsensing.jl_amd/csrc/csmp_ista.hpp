// csmp_ista.hpp -- gfx950 kernels of the proximal-gradient path: ista(A, b, w, x) (src/basispursuit.jl:164-183) and the
// Beck-Teboulle FISTA on the same objective  ||b - A x||^2 + sum_j w_j |x_j|.
//
// One iteration is   r = b - A y;   c = A' r (the product sweep of csmp_kernels.hpp, unchanged);
//                    x+ = shrinkage(y + 2 alpha c, w alpha);   y+ = x+ + beta (x+ - x)     (beta = 0: ISTA, y = x).
//   k_ista_update   the element-wise step over the N atoms, and the list of the non-zeros of the next y
//   k_ista_axpy     r's subtrahend  sum_j y_j a_j  over that list, one partial M-vector per workgroup
//   k_ista_resum    r = b - (the partials, added in a fixed order)
// The list has any length from 0 to N: with a small l1 weight most atoms are alive and k_ista_axpy reads as many bytes of A as
// the sweep does, so it is built like the sweep (whole contiguous column pieces, 16-byte non-temporal loads, a ring of loads in
// flight per wave, Float64 accumulators in registers).
//
// Determinism: the list is in ascending index order, the split of the list over the workgroups depends on its length only, a
// workgroup adds its columns in list order and k_ista_resum adds the workgroups' partials in workgroup order -- no atomics, the
// same bits on every run.
#pragma once
#include "csmp_kernels.hpp"

namespace csmp {

constexpr int kIstaThreads = 256;
constexpr int kIstaMaxSegs = 1024;  // segments of the list (one k_ista_update workgroup each)
constexpr int kIstaTile = 256;      // list entries a k_ista_axpy workgroup stages in the LDS at a time
constexpr int kIstaL = 4;           // 16-byte loads per lane and column: a wave owns 4 KiB of a column
constexpr int kIstaNB = 4;          // columns in flight per wave (a ring of kIstaNB * kIstaL loads)
constexpr int kIstaMinCols = 8;     // a further workgroup takes part only once every one of them has this many columns
enum : int { ISTA_ACCEL = 1, ISTA_INIT = 2, ISTA_LIST_X = 4 };

// The list is kept in SEGMENTS: workgroup s of k_ista_update owns the atoms [s * seg_len, (s + 1) * seg_len), writes their
// non-zeros in ascending order from entry s * seg_len on and their number to seg_cnt[s].  Entry p of the list as a whole is entry
// p - off[s] of the segment with off[s] <= p < off[s + 1], off = the exclusive scan of seg_cnt: every reader computes that scan
// itself (at most 1024 numbers, in a fixed order) -- the writers never wait for one another.
// off: nseg + 1 words, ws: 256 words of LDS.  Returns the list's length; ends with a barrier.
__device__ __forceinline__ unsigned ista_seg_scan(const int* __restrict__ seg_cnt, int nseg, unsigned* off, unsigned* ws) {
    const int t = threadIdx.x;
    unsigned c[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * t + q;
        c[q] = i < nseg ? (unsigned)seg_cnt[i] : 0u;
        s += c[q];
    }
    ws[t] = s;
    __syncthreads();
    for (int d = 1; d < kIstaThreads; d <<= 1) {
        const unsigned v = t >= d ? ws[t - d] : 0u;
        __syncthreads();
        ws[t] += v;
        __syncthreads();
    }
    unsigned base = ws[t] - s;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * t + q;
        if (i < nseg) off[i] = base;
        base += c[q];
    }
    if (t == kIstaThreads - 1) off[nseg] = ws[t];
    __syncthreads();
    return off[nseg];
}
// workgroups that share a list of n columns, of the P the launch has
__host__ __device__ __forceinline__ int ista_parts(unsigned n, int P) {
    const unsigned want = (n + kIstaMinCols - 1) / kIstaMinCols;
    return want < (unsigned)P ? (int)want : P;
}

// x+ = sign(u) max(|u| - w alpha, 0), u = y + 2 alpha c (src/basispursuit.jl:144,179); y+ = x+ + beta (x+ - x) under ISTA_ACCEL,
// else y+ = x+.  An exact zero is a structural zero (dropzeros!, :180): it is not listed.  ISTA_INIT: x = y as it stands (the warm
// start), no step.  ISTA_LIST_X: the list is that of x+ instead of y+ (the last iteration: the residual of the RESULT follows).
// The body is shared with k_ista_update_group (csmp_bp.hpp).  (seg: the workgroup's segment)
__device__ __forceinline__ void ista_update_body(const unsigned seg, const double* __restrict__ c, const double* __restrict__ w, int64_t nw,
                                                 double* __restrict__ x, double* __restrict__ y, int64_t N, int64_t seg_len, double alpha,
                                                 double beta, int flags, int* __restrict__ lidx, double* __restrict__ lval,
                                                 int* __restrict__ seg_cnt) {
    __shared__ int wcnt[kIstaThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j0 = (int64_t)seg * seg_len, j1 = j0 + seg_len < N ? j0 + seg_len : N;
    const double w0 = w[0];
    int64_t base = j0;
    for (int64_t jt = j0; jt < j1; jt += kIstaThreads) {
        const int64_t j = jt + tid;
        double lv = 0.0;
        if (j < j1) {
            const double yv = y[j];
            double xn = yv, yn = yv;
            if (!(flags & ISTA_INIT)) {
                const double u = yv + 2.0 * alpha * c[j];
                const double m = fabs(u) - (nw == 1 ? w0 : w[j]) * alpha;
                xn = m > 0.0 ? copysign(m, u) : 0.0;
                yn = (flags & ISTA_ACCEL) ? xn + beta * (xn - x[j]) : xn;
            }
            x[j] = xn;
            y[j] = yn;
            lv = (flags & ISTA_LIST_X) ? xn : yn;
        }
        const bool nz = lv != 0.0;
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
            lval[p] = lv;
        }
        base += all;
        __syncthreads();
    }
    if (tid == 0) seg_cnt[seg] = (int)(base - j0);
}
__global__ __launch_bounds__(kIstaThreads) void k_ista_update(const double* __restrict__ c, const double* __restrict__ w, int64_t nw,
                                                              double* __restrict__ x, double* __restrict__ y, int64_t N, int64_t seg_len,
                                                              double alpha, double beta, int flags, int* __restrict__ lidx,
                                                              double* __restrict__ lval, int* __restrict__ seg_cnt) {
    ista_update_body(blockIdx.x, c, w, nw, x, y, N, seg_len, alpha, beta, flags, lidx, lval, seg_cnt);
}

// part[p] = sum over workgroup p's share of the list of  val_t * A[:, idx_t]  (Float64 on the promoted entries), for the row block
// blockIdx.y: kIstaThreads / 64 waves x 64 lanes x kIstaL vectors of 16 bytes.  Grid (P, row blocks): P comes from the device's
// size, not from the list -- the workgroups beyond ista_parts(n, P) leave at once, and k_ista_resum adds that many partials.
// Ragged columns: a lane past the column's end re-reads the column's last vector (valid memory, no predicate in the load stream)
// and its sums are not stored; a wave wholly past the end loads nothing.
// The body is shared with k_ista_axpy_group (csmp_bp.hpp): it reads blockIdx.x / .y and gridDim.x only.
template <typename TA>
__device__ __forceinline__ void ista_axpy_body(const TA* __restrict__ A, int64_t ld, int Mv, const int* __restrict__ seg_cnt,
                                               int nseg, int64_t seg_len, const int* __restrict__ lidx,
                                               const double* __restrict__ lval, double* __restrict__ part,
                                               unsigned* __restrict__ nnz_out) {
    using VT = typename Vec<TA>::type;
    constexpr int VEC = Vec<TA>::n, L = kIstaL, NB = kIstaNB;
    __shared__ unsigned off[kIstaMaxSegs + 1];
    __shared__ unsigned ws[kIstaThreads];
    __shared__ int tidx[kIstaTile];
    __shared__ double tval[kIstaTile];
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
    double acc[L * VEC];
#pragma unroll
    for (int q = 0; q < L * VEC; ++q) acc[q] = 0.0;
    auto issue = [&](VT(&b)[L], int i) {
        const int j = __builtin_amdgcn_readfirstlane(tidx[i]);
        const VT* pc = reinterpret_cast<const VT*>(A + (int64_t)j * ld);
#pragma unroll
        for (int q = 0; q < L; ++q) b[q] = __builtin_nontemporal_load(pc + vq[q]);
    };
    auto consume = [&](const VT(&b)[L], int i) {
        const double yv = tval[i];
#pragma unroll
        for (int q = 0; q < L; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q * VEC + e] = fma((double)b[q][e], yv, acc[q * VEC + e]);
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
            tval[tid] = lval[e];
        }
        __syncthreads();
        if (!active) continue;
        // the ring: kIstaNB columns in flight, a consumed buffer is refilled at once with the column kIstaNB ahead
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
        for (int d = 0; d < NB; ++d) {  // the last kIstaNB .. 2 kIstaNB - 1 columns of the tile (or all of them, when there are fewer)
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
    double* out = part + (int64_t)p * Mv;
#pragma unroll
    for (int q = 0; q < L; ++q) {
        const int v = v0 + q * kWave + lane;
        if (v < nvec) {
#pragma unroll
            for (int e = 0; e < VEC; e += 2) {
                f64x2 s2;
                s2.x = acc[q * VEC + e];
                s2.y = acc[q * VEC + e + 1];
                *reinterpret_cast<f64x2*>(out + (int64_t)v * VEC + e) = s2;
            }
        }
    }
}
template <typename TA>
__global__ __launch_bounds__(kIstaThreads) void k_ista_axpy(const TA* __restrict__ A, int64_t ld, int Mv, const int* __restrict__ seg_cnt,
                                                            int nseg, int64_t seg_len, const int* __restrict__ lidx,
                                                            const double* __restrict__ lval, double* __restrict__ part,
                                                            unsigned* __restrict__ nnz_out) {
    ista_axpy_body<TA>(A, ld, Mv, seg_cnt, nseg, seg_len, lidx, lval, part, nnz_out);
}

// r = b - (part[0] + part[1] + ... ), the first ista_parts(n, P) partials: a workgroup takes 64 rows, its four waves a quarter
// of the partials each (in order), and the four sums are added as (s0 + s1) + (s2 + s3).  n = 0: r = b.
__device__ __forceinline__ void ista_resum_body(const double* __restrict__ part, int Mv, int M, const unsigned* __restrict__ nnz,
                                                int P, const double* __restrict__ b, double* __restrict__ r) {
    __shared__ double red[kIstaThreads / kWave][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Pa = ista_parts(*nnz, P);
    const int row = blockIdx.x * kWave + lane;
    double s = 0.0;
    if (row < M)
        for (int p = wave * Pa / 4; p < (wave + 1) * Pa / 4; ++p) s += part[(int64_t)p * Mv + row];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && row < M) r[row] = b[row] - ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
}

__global__ __launch_bounds__(kIstaThreads) void k_ista_resum(const double* __restrict__ part, int Mv, int M, const unsigned* __restrict__ nnz,
                                                             int P, const double* __restrict__ b, double* __restrict__ r) {
    ista_resum_body(part, Mv, M, nnz, P, b, r);
}

}  // namespace csmp
