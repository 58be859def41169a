// csmp_bp.hpp -- gfx950 kernels of basis pursuit, basispursuit(A, b[, w]) (src/basispursuit.jl:1-16):  min sum_j w_j |x_j|  s.t.  A x = b,
// by ADMM on the split x = z (include/csmp.h, csmp_bp).  With G = A A' = R'R, scaled dual u, penalty rho, p = A z and q = A u:
//     e = p - q - b;   y = R^-1 (R^-T e);   c = A' y (the product sweep);   t = z - c
//     z+ = shrink(t, w / rho);   u+ = t - z+;   r = b - A z+ (k_ista_axpy / k_ista_resum over the list of z+)
//     p+ = b - r;   q+ = p - G y - p+
//   k_rowgram          G = A A' on the Float64 matrix cores, straight from the resident dictionary (no transposed copy): upper
//                      128 x 128 tiles, the N columns split over workgroups, one partial M x M matrix per split
//   k_rowgram_reduce   the partials added in split order; writes the full symmetric G
//   k_bp_assemble      [G | I] in the layout the blocked Cholesky of csmp_gram.hpp factorises: R^-T comes out beside R
//   k_bp_transpose     R^-1 (upper) from R^-T (lower), into the rows of the augmented matrix the factorisation never touches
//   k_bp_gemv          one triangular or full M x M matrix-vector product, a wave per output, along contiguous columns
//   k_bp_start / k_bp_pq   the M-vector steps
//   k_bp_update        the element-wise step over the N atoms, the list of z+ (k_ista_update's layout), the residual norms' partials
//   k_bp_fold          the partials added in segment order
//   k_bp_gemm          k_bp_gemv for up to eight right-hand sides per read of the matrix, and the group forms k_bp_update_group,
//                      k_ista_axpy_group, k_ista_resum_group, k_bp_pq_group: csmp_bp_batch's step for all live members (host/bp_batch.hpp)
//   k_ista_update_group  k_ista_update for the members of a group of csmp_ista_batch (host/ista_batch.hpp)
//
// Determinism: no atomics, no workgroup waits for another, every sum has a fixed order: the same bits on every run.
#pragma once
#include "csmp_gram.hpp"
#include "csmp_ista.hpp"

namespace csmp {

constexpr int kRgTile = 128;              // G tile edge per workgroup: 2 x 2 waves, each 64 x 64 = 4 x 4 MFMA tiles
constexpr int kRgKC = 16;                 // dictionary columns per stage
constexpr int kRgStride = kRgTile + 16;   // doubles per staged column: a ds_read_b64 serves lanes 0..31 at once, 16 consecutive rows of
                                          // two columns -- 144 * 8 B = 4 * 256 + 128 puts the second column on the other 32 banks
constexpr int kRgMinCols = 256;           // a further column split only where every split keeps this many columns
constexpr int kRgMaxSplit = 64;
__host__ __device__ constexpr size_t rowgram_lds_bytes() { return (size_t)2 * 2 * kRgKC * kRgStride * sizeof(double); }

// Gpart[split] (M x M, leading dimension M): the upper tile blockIdx.x = (I, J), I <= J, of  sum over the split's columns of a_c a_c'
// (a_c = column c of the dictionary, promoted exactly).  A stage is kRgKC columns x 128 rows of both row blocks in the LDS as
// doubles, column after column (rows contiguous, as in memory); MFMA step kk multiplies columns 4 kk + (lane >> 4) of both
// operands.  Double-buffered: the next stage's loads are in flight under the current stage's 64 MFMAs per wave.  Rows beyond M and
// columns beyond the split's end are loaded from clamped addresses and staged as zeros; stores are masked.  VEC: the columns start
// on 16-byte boundaries -- 16-byte loads wherever the vector lies inside the column.  A diagonal tile stages one block.
// WT (csmp_sbl.hpp): the sum is weighted,  sum gam[c] a_c a_c' -- the second operand is scaled by gam[c] as it is staged (one rounding
// per entry), so a diagonal tile stages both blocks too.  WT = false reads no gam and does what it did before the flag existed.
template <typename TA, bool VEC, bool WT = false>
__global__ __launch_bounds__(256) void k_rowgram(const TA* __restrict__ A, int64_t ld, int M, int64_t N, int64_t cols_per_split,
                                                 double* __restrict__ Gpart, const double* __restrict__ gam = nullptr) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    typedef TA tav __attribute__((ext_vector_type(16 / sizeof(TA))));
    constexpr int PERV = 16 / (int)sizeof(TA), GPC = kRgTile / PERV, NQ = kRgKC * GPC / 256, S = kRgStride;
    extern __shared__ __attribute__((aligned(16))) double rglds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int wi = wave >> 1, wj = wave & 1;
    int J = 0;
    while ((J + 1) * (J + 2) / 2 <= (int)blockIdx.x) ++J;
    const int I = (int)blockIdx.x - J * (J + 1) / 2;
    const bool diag = I == J;
    const int64_t c0 = (int64_t)blockIdx.y * cols_per_split, c1 = c0 + cols_per_split < N ? c0 + cols_per_split : N;
    const int nst = (int)((c1 - c0 + kRgKC - 1) / kRgKC);
    const bool one = diag && !WT;  // both operands are the same staged block
    const int nop = one ? 1 : 2;
    TA raw[2][NQ][PERV];
    double gw[NQ];
    d4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};

    auto fetch = [&](int st) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h >= nop) continue;
            const int rb = (h ? J : I) * kRgTile;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int g = tid + 256 * q, cl = g / GPC, r = rb + (g % GPC) * PERV;
                const int64_t c = c0 + (int64_t)st * kRgKC + cl;
                const TA* col = A + (c < c1 ? c : c1 - 1) * ld;
                if (WT && h == 1) gw[q] = gam[c < c1 ? c : c1 - 1];
                if (VEC && r + PERV <= M) {
                    const tav x = *reinterpret_cast<const tav*>(col + r);
#pragma unroll
                    for (int e = 0; e < PERV; ++e) raw[h][q][e] = x[e];
                } else {
#pragma unroll
                    for (int e = 0; e < PERV; ++e) raw[h][q][e] = col[r + e < M ? r + e : M - 1];
                }
            }
        }
    };
    auto store = [&](int buf, int st) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h >= nop) continue;
            const int rb = (h ? J : I) * kRgTile;
            double* dst = rglds + (size_t)(buf * 2 + h) * kRgKC * S;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int g = tid + 256 * q, cl = g / GPC, rl = (g % GPC) * PERV;
                const bool colok = c0 + (int64_t)st * kRgKC + cl < c1;
#pragma unroll
                for (int e = 0; e < PERV; e += 2) {
                    f64x2 v;
                    v.x = (colok && rb + rl + e < M) ? (double)raw[h][q][e] : 0.0;
                    v.y = (colok && rb + rl + e + 1 < M) ? (double)raw[h][q][e + 1] : 0.0;
                    if (WT && h == 1) {
                        v.x *= gw[q];
                        v.y *= gw[q];
                    }
                    *reinterpret_cast<f64x2*>(dst + cl * S + rl + e) = v;
                }
            }
        }
    };
    auto compute = [&](int buf) {
        const double* pa = rglds + (size_t)(buf * 2) * kRgKC * S + wi * 64 + fr;
        const double* pb = rglds + (size_t)(buf * 2 + (one ? 0 : 1)) * kRgKC * S + wj * 64 + fr;
#pragma unroll
        for (int kk = 0; kk < kRgKC / 4; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = pa[(kk * 4 + fq) * S + t * 16];
                b[t] = pb[(kk * 4 + fq) * S + t * 16];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[u], acc[t][u], 0, 0, 0);
        }
    };

    if (nst > 0) {
        fetch(0);
        store(0, 0);
    }
    __syncthreads();
    int buf = 0;
    for (int st = 0; st < nst; ++st) {
        const bool more = st + 1 < nst;
        if (more) fetch(st + 1);
        compute(buf);
        if (more) store(buf ^ 1, st + 1);
        __syncthreads();
        buf ^= 1;
    }
    // C/D layout: column = lane & 15, row = (lane >> 4) + 4 reg
    double* out = Gpart + (int64_t)blockIdx.y * M * M;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = I * kRgTile + wi * 64 + t * 16 + fq + 4 * reg, col = J * kRgTile + wj * 64 + u * 16 + fr;
                if (row < M && col < M) out[row + (int64_t)col * M] = acc[t][u][reg];
            }
}

// G (M x M, full): entry (row, col) = the sum of the partials at (min, max), in split order -- exactly symmetric
__global__ __launch_bounds__(256) void k_rowgram_reduce(const double* __restrict__ Gpart, int nsplit, int M, double* __restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)M * M) return;
    const int row = (int)(e % M), col = (int)(e / M);
    const int64_t u = min(row, col) + (int64_t)max(row, col) * M;
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += Gpart[(int64_t)q * M * M + u];
    G[e] = s;
}

// Gm (leading dimension npa = 2 np, rows [0, np)): columns [0, np) hold G, the identity on the padding diagonal; columns [np, np + M)
// the unit vectors -- the row panels of the factorisation leave R^-T there (csmp_gram.hpp, the augmented form).  pivref[i] =
// 2 thr G_ii: the Cholesky kernels accept a pivot d only when d > 0 and d >= pivref / 2, "positive to working precision".
__global__ __launch_bounds__(256) void k_bp_assemble(const double* __restrict__ G, int M, int np, int npa, double thr, double* __restrict__ Gm,
                                                     double* __restrict__ pivref) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)npa * npa) return;
    const int row = (int)(e % npa), col = (int)(e / npa);
    if (row >= np) return;
    double v;
    if (col < np) {
        v = (row < M && col < M) ? G[row + (int64_t)col * M] : (row == col ? 1.0 : 0.0);
        if (row == col) pivref[row] = row < M ? 2.0 * thr * v : 0.0;
    } else {
        v = (row < M && row == col - np) ? 1.0 : 0.0;
    }
    Gm[e] = v;
}

// Ri[i, j] = T[j, i] for i <= j < M (T = R^-T lower triangular, Ri = R^-1 upper), both with leading dimension ld; 32 x 32 tiles
// through the LDS, tiles above T's diagonal are skipped
__global__ __launch_bounds__(256) void k_bp_transpose(const double* __restrict__ T, int64_t ld, int M, double* __restrict__ Ri) {
    __shared__ double tile[32][33];
    const int bj = blockIdx.x, bi = blockIdx.y;  // T's tile (rows 32 bj .., columns 32 bi ..)
    if (bi > bj) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = bj * 32 + tx, i = bi * 32 + ty + 8 * q;
        tile[ty + 8 * q][tx] = (j < M && i <= j) ? T[j + (int64_t)i * ld] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = bi * 32 + tx, j = bj * 32 + ty + 8 * q;
        if (j < M && i <= j) Ri[i + (int64_t)j * ld] = tile[tx][ty + 8 * q];
    }
}

// out[c] = sum_t mat[t, c] x[t] over t in [0, c] (BP_UPPER), [c, M) (BP_LOWER) or [0, M) (BP_FULL): column c is contiguous.  One wave
// per output (k_tt_gemv's scheme): lane partials in row order, two chains, then the butterfly.
enum : int { BP_UPPER = 0, BP_LOWER = 1, BP_FULL = 2 };
__global__ __launch_bounds__(256) void k_bp_gemv(const double* __restrict__ mat, int64_t ld, int M, int mode, const double* __restrict__ x,
                                                 double* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= M) return;
    const int lo = mode == BP_LOWER ? c : 0, hi = mode == BP_UPPER ? c + 1 : M;
    const double* col = mat + (int64_t)c * ld;
    double a0 = 0.0, a1 = 0.0;
    int t = lo + lane;
    for (; t + 64 < hi; t += 128) {
        a0 = fma(col[t], x[t], a0);
        a1 = fma(col[t + 64], x[t + 64], a1);
    }
    if (t < hi) a0 = fma(col[t], x[t], a0);
    double a = a0 + a1;
    for (int s = 32; s >= 1; s >>= 1) a += shx(a, s);
    if (lane == 0) out[c] = a;
}

// k_bp_gemv for the L right-hand sides of one step of csmp_bp_batch (host/bp_batch.hpp):  out_m[c] = sum_t mat[t, c] x_m[t],  m < L.
// A wave per output column as above; a lane loads its matrix elements ONCE and feeds each to L fmas, so a launch's traffic from
// memory is one pass over the triangle or the square whatever L is (the L vectors, L M doubles, stay in the caches).  For every pair
// (c, m) the operations are k_bp_gemv's and nothing else -- the lane partials over t = lo + lane in steps of 128 on the chains a0 and
// a1, the tail into a0, a0 + a1, the butterfly 32 .. 1 -- so every out_m has k_bp_gemv's bits; L = 1 is k_bp_gemv.
// 2 L accumulators per column, 2 + 2 L loads in flight per lane and trip, no LDS, no scratch.
constexpr int kBpGemmMax = 8;
struct BpGemm {
    const double* x[kBpGemmMax];
    double* out[kBpGemmMax];
};
template <int L>
__global__ __launch_bounds__(256) void k_bp_gemm(const double* __restrict__ mat, int64_t ld, int M, int mode, const BpGemm g) {
    static_assert(L >= 1 && L <= kBpGemmMax, "right-hand sides of a launch");
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= M) return;
    const int lo = mode == BP_LOWER ? c : 0, hi = mode == BP_UPPER ? c + 1 : M;
    const double* col = mat + (int64_t)c * ld;
    double a0[L], a1[L];
#pragma unroll
    for (int m = 0; m < L; ++m) a0[m] = a1[m] = 0.0;
    int t = lo + lane;
    for (; t + 64 < hi; t += 128) {
        const double m0 = col[t], m1 = col[t + 64];
        double x0[L], x1[L];
#pragma unroll
        for (int m = 0; m < L; ++m) {
            x0[m] = g.x[m][t];
            x1[m] = g.x[m][t + 64];
        }
#pragma unroll
        for (int m = 0; m < L; ++m) {
            a0[m] = fma(m0, x0[m], a0[m]);
            a1[m] = fma(m1, x1[m], a1[m]);
        }
    }
    if (t < hi) {
        const double m0 = col[t];
#pragma unroll
        for (int m = 0; m < L; ++m) a0[m] = fma(m0, g.x[m][t], a0[m]);
    }
#pragma unroll
    for (int m = 0; m < L; ++m) {
        double a = a0[m] + a1[m];
        for (int s = 32; s >= 1; s >>= 1) a += shx(a, s);
        if (lane == 0) g.out[m][c] = a;
    }
}

// the start from z = u = 0:  p = q = 0,  e = -b
__global__ __launch_bounds__(256) void k_bp_start(const double* __restrict__ b, int M, double* __restrict__ p, double* __restrict__ q,
                                                  double* __restrict__ e) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    p[i] = 0.0;
    q[i] = 0.0;
    e[i] = -b[i];
}
// p+ = b - r;  q+ = p - g - p+ (g = G y);  and the next iteration's  e = p+ - q+ - b.  blk: the workgroup's 256 rows.
__device__ __forceinline__ void bp_pq_body(const int blk, const double* __restrict__ b, const double* __restrict__ r, const double* __restrict__ g,
                                           int M, double* __restrict__ p, double* __restrict__ q, double* __restrict__ e) {
    const int i = blk * 256 + threadIdx.x;
    if (i >= M) return;
    const double pn = b[i] - r[i];
    const double qn = p[i] - g[i] - pn;
    p[i] = pn;
    q[i] = qn;
    e[i] = pn - qn - b[i];
}
__global__ __launch_bounds__(256) void k_bp_pq(const double* __restrict__ b, const double* __restrict__ r, const double* __restrict__ g, int M,
                                               double* __restrict__ p, double* __restrict__ q, double* __restrict__ e) {
    bp_pq_body((int)blockIdx.x, b, r, g, M, p, q, e);
}

// t = z - c;  z+ = sign(t) max(|t| - w / rho, 0);  u+ = t - z+.  The list is that of z+, in k_ista_update's layout (segments of seg_len
// atoms, one workgroup each, seg_cnt): k_ista_axpy consumes it unchanged.  rpart[s] = the segment's share of |u+ - u|^2,
// rpart[kIstaMaxSegs + s] of |z+ - z|^2 (thread partials in index order, then block_sum256).
// (seg: the workgroup's segment)
__device__ __forceinline__ void bp_update_body(const int seg, const double* __restrict__ c, const double* __restrict__ w, int64_t nw, double rho,
                                               double* __restrict__ z, double* __restrict__ u, int64_t N, int64_t seg_len,
                                               int* __restrict__ lidx, double* __restrict__ lval, int* __restrict__ seg_cnt,
                                               double* __restrict__ rpart) {
    __shared__ int wcnt[kIstaThreads / kWave];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j0 = (int64_t)seg * seg_len, j1 = j0 + seg_len < N ? j0 + seg_len : N;
    const double w0 = w[0];
    double sp = 0.0, sd = 0.0;
    int64_t base = j0;
    for (int64_t jt = j0; jt < j1; jt += kIstaThreads) {
        const int64_t j = jt + tid;
        double zn = 0.0;
        if (j < j1) {
            const double zo = z[j], uo = u[j];
            const double t = zo - c[j];
            const double m = fabs(t) - (nw == 1 ? w0 : w[j]) / rho;
            zn = m > 0.0 ? copysign(m, t) : 0.0;
            const double un = t - zn;
            z[j] = zn;
            u[j] = un;
            const double du = un - uo, dz = zn - zo;
            sp = fma(du, du, sp);
            sd = fma(dz, dz, sd);
        }
        const bool nz = zn != 0.0;
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
            lval[p] = zn;
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
__global__ __launch_bounds__(kIstaThreads) void k_bp_update(const double* __restrict__ c, const double* __restrict__ w, int64_t nw, double rho,
                                                            double* __restrict__ z, double* __restrict__ u, int64_t N, int64_t seg_len,
                                                            int* __restrict__ lidx, double* __restrict__ lval, int* __restrict__ seg_cnt,
                                                            double* __restrict__ rpart) {
    bp_update_body((int)blockIdx.x, c, w, nw, rho, z, u, N, seg_len, lidx, lval, seg_cnt, rpart);
}

// ---------------------------------------------------------------------------------------------
// The group forms of csmp_bp_batch (host/bp_batch.hpp): ONE launch does a kernel's work for every live member of a lockstep group.
// The member is the grid's third axis; its pointers come from this kernel-argument struct (the live members in entries [0, n), in
// slot order).  Every member's workgroups run the single kernels' bodies above (and ista_axpy_body / ista_resum_body, csmp_ista.hpp)
// on the member's own buffers: per member the arithmetic and its order are the single solve's.  The weights are shared.
constexpr int kBpGroupMax = 8;
struct BpGroup {
    int n;
    const double* c[kBpGroupMax];                                                  // the pass's c = A'y (the member's slot)
    double *z[kBpGroupMax], *u[kBpGroupMax];                                       // the iterates
    int *lidx[kBpGroupMax], *seg_cnt[kBpGroupMax]; double* lval[kBpGroupMax];      // the list of z+
    double* rpart[kBpGroupMax];                                                    // the residual norms' partials
    double* part[kBpGroupMax]; unsigned* nnz[kBpGroupMax];                         // the axpy's partials and the list's length
    const double* b[kBpGroupMax]; double* r[kBpGroupMax];                          // the member's slot
    const double* g[kBpGroupMax]; double *p[kBpGroupMax], *q[kBpGroupMax], *e[kBpGroupMax];
};
static_assert(sizeof(BpGroup) <= 4096, "kernel arguments");
__global__ __launch_bounds__(kIstaThreads) void k_bp_update_group(const BpGroup G, const double* __restrict__ w, int64_t nw, double rho, int64_t N,
                                                                  int64_t seg_len) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    bp_update_body((int)blockIdx.x, G.c[m], w, nw, rho, G.z[m], G.u[m], N, seg_len, G.lidx[m], G.lval[m], G.seg_cnt[m], G.rpart[m]);
}
template <typename TA>
__global__ __launch_bounds__(kIstaThreads) void k_ista_axpy_group(const TA* __restrict__ A, int64_t ld, int Mv, int nseg, int64_t seg_len,
                                                                  const BpGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    ista_axpy_body<TA>(A, ld, Mv, G.seg_cnt[m], nseg, seg_len, G.lidx[m], G.lval[m], G.part[m], G.nnz[m]);
}
__global__ __launch_bounds__(kIstaThreads) void k_ista_resum_group(int Mv, int M, int P, const BpGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    ista_resum_body(G.part[m], Mv, M, G.nnz[m], P, G.b[m], G.r[m]);
}
__global__ __launch_bounds__(256) void k_bp_pq_group(int M, const BpGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    bp_pq_body((int)blockIdx.x, G.b[m], G.r[m], G.g[m], M, G.p[m], G.q[m], G.e[m]);
}
// csmp_ista_batch's step (host/ista_batch.hpp): k_ista_update for every member of a group, x in z's place and y in u's.  Here every
// member has weights of its own (W.w[m]: nw of them; the members of a batch with shared weights point at one set); alpha, beta and the
// flags are the group's -- all members are at the same iteration.
struct IstaGroupW {
    const double* w[kBpGroupMax];
};
__global__ __launch_bounds__(kIstaThreads) void k_ista_update_group(const BpGroup G, const IstaGroupW W, int64_t nw, int64_t N, int64_t seg_len,
                                                                    double alpha, double beta, int flags) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    ista_update_body(blockIdx.x, G.c[m], W.w[m], nw, G.z[m], G.u[m], N, seg_len, alpha, beta, flags, G.lidx[m], G.lval[m], G.seg_cnt[m]);
}

// res[0] = |u+ - u|^2, res[1] = |z+ - z|^2: the nseg <= 1024 partials of each, four per thread in order, then block_sum256
__global__ __launch_bounds__(256) void k_bp_fold(const double* __restrict__ rpart, int nseg, double* __restrict__ res) {
    __shared__ double red[4];
    double s[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * threadIdx.x + q;
            if (i < nseg) v += rpart[h * kIstaMaxSegs + i];
        }
        s[h] = block_sum256(v, red);
    }
    if (threadIdx.x == 0) {
        res[0] = s[0];
        res[1] = s[1];
    }
}

}  // namespace csmp
