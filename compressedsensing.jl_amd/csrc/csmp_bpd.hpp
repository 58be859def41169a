// csmp_bpd.hpp -- gfx950 kernels of basis pursuit denoising, basis_pursuit_denoising(A, b, delta[, w]) (src/basispursuit.jl:76-124):
// min sum_j w_j |x_j|  s.t.  |A x - b|_2 <= delta,  by graph-form ADMM (include/csmp.h, csmp_bpd).  Block one is (x, s) on s = A x, block
// two (z, v) with the l1 term and the ball; scaled duals u (x = z) and lam (s = v), penalty rho, K = I + A A' = R'R, p = A z, q = A u:
//     e = v - lam - p + q;   y = R^-1 (R^-T e);   c = A' y (the product sweep);   t = z + c
//     z+ = shrink(t, w / rho);   u+ = t - z+;   r = b - A z+ (k_ista_axpy / k_ista_resum over the list of z+)
//     p+ = b - r;   q+ = p + (e - y) - p+                    (A A' y = (K - I) y = e - y: no product with A A')
//     h = v - y - b;   v+ = b + h min(1, delta / |h|);   lam+ = v - y - v+
// The iteration carries the NEGATED e and y (en, yn): the two triangular products are linear, the sweep of yn gives -c, and k_bp_update's
// t = z - (-c) is the t above -- that kernel, k_bp_gemv, k_bp_transpose, k_rowgram and the Cholesky launches are csmp_bp's, unchanged.
//   k_bpd_assemble     [K | I], K = G + I, in the layout the blocked Cholesky factorises (k_bp_assemble's, G's diagonal raised by one)
//   k_bpd_start        the start from zeros
//   k_bpd_pq           p+, q+, h, and one partial of |h|^2 per workgroup
//   k_bpd_ball         every workgroup adds the partials of |h|^2 in index order (the same bits in each), then v+, lam+, the next en, and
//                      one partial each of |lam+ - lam|^2 and |v+ - v|^2
//   k_bpd_fold         the four sums of the stopping test, partials added in index order
//   k_bpd_pq_group, k_bpd_ball_group   the two M-vector kernels for every live member of csmp_bpd_batch's group in one launch each
//
// Determinism: no atomics, no workgroup waits for another, every sum has a fixed order: the same bits on every run.
#pragma once
#include "csmp_bp.hpp"

namespace csmp {

constexpr int kBpdMaxParts = 2048;  // workgroups of the M-vector stage: 2^19 rows / 256

// k_bp_assemble with K = G + I: Gm columns [0, np) hold K (the identity on the padding diagonal), columns [np, np + M) the unit vectors;
// pivref[i] = 2 thr K_ii.  K's smallest eigenvalue is at least 1: a refused pivot is a fault of the factorisation, not of the dictionary.
__global__ __launch_bounds__(256) void k_bpd_assemble(const double* __restrict__ G, int M, int np, int npa, double thr, double* __restrict__ Gm,
                                                      double* __restrict__ pivref) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)npa * npa) return;
    const int row = (int)(e % npa), col = (int)(e / npa);
    if (row >= np) return;
    double v;
    if (col < np) {
        v = (row < M && col < M) ? G[row + (int64_t)col * M] + (row == col ? 1.0 : 0.0) : (row == col ? 1.0 : 0.0);
        if (row == col) pivref[row] = row < M ? 2.0 * thr * v : 0.0;
    } else {
        v = (row < M && row == col - np) ? 1.0 : 0.0;
    }
    Gm[e] = v;
}

// the start from z = u = 0, v = lam = 0:  p = q = 0,  en = 0
__global__ __launch_bounds__(256) void k_bpd_start(int M, double* __restrict__ p, double* __restrict__ q, double* __restrict__ v,
                                                   double* __restrict__ lam, double* __restrict__ en) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    p[i] = 0.0;
    q[i] = 0.0;
    v[i] = 0.0;
    lam[i] = 0.0;
    en[i] = 0.0;
}

// p+ = b - r;  q+ = p + (e - y) - p+ = p - (en - yn) - p+;  h = v - y - b = v + yn - b;  hpart[workgroup] = its share of |h|^2 (thread
// squares in index order through block_sum256; rows beyond M add zeros).  blk: the workgroup's 256 rows.
__device__ __forceinline__ void bpd_pq_body(const int blk, const double* __restrict__ b, const double* __restrict__ r, const double* __restrict__ en,
                                            const double* __restrict__ yn, const double* __restrict__ v, int M, double* __restrict__ p,
                                            double* __restrict__ q, double* __restrict__ h, double* __restrict__ hpart) {
    __shared__ double red[4];
    const int i = blk * 256 + threadIdx.x;
    double hh = 0.0;
    if (i < M) {
        const double pn = b[i] - r[i];
        q[i] = p[i] - (en[i] - yn[i]) - pn;
        p[i] = pn;
        hh = v[i] + yn[i] - b[i];
        h[i] = hh;
    }
    const double s = block_sum256(hh * hh, red);
    if (threadIdx.x == 0) hpart[blk] = s;
}
__global__ __launch_bounds__(256) void k_bpd_pq(const double* __restrict__ b, const double* __restrict__ r, const double* __restrict__ en,
                                                const double* __restrict__ yn, const double* __restrict__ v, int M, double* __restrict__ p,
                                                double* __restrict__ q, double* __restrict__ h, double* __restrict__ hpart) {
    bpd_pq_body((int)blockIdx.x, b, r, en, yn, v, M, p, q, h, hpart);
}

// |h|^2 = the nparts <= kBpdMaxParts partials, eight per thread in index order, then block_sum256 -- the same operations in every
// workgroup, so every workgroup scales by the same bits.  v+ = b + h delta / |h| where |h| > delta, else b + h (h = 0 and delta = 0
// included);  lam+ = v + yn - v+;  the next iteration's  en = -(v+ - lam+ - p+ + q+).  mpart[workgroup] = its share of |lam+ - lam|^2,
// mpart[kBpdMaxParts + workgroup] of |v+ - v|^2.
__device__ __forceinline__ void bpd_ball_body(const int blk, const double* __restrict__ b, const double* __restrict__ h, const double* __restrict__ yn,
                                              const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ hpart,
                                              int nparts, double delta, int M, double* __restrict__ v, double* __restrict__ lam,
                                              double* __restrict__ en, double* __restrict__ mpart) {
    __shared__ double red[4];
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < kBpdMaxParts / 256; ++k) {
        const int j = (kBpdMaxParts / 256) * threadIdx.x + k;
        if (j < nparts) a += hpart[j];
    }
    const double nh = sqrt(block_sum256(a, red));
    const double scale = nh > delta ? delta / nh : 1.0;
    const int i = blk * 256 + threadIdx.x;
    double dl = 0.0, dv = 0.0;
    if (i < M) {
        const double vo = v[i], lo = lam[i];
        const double vn = b[i] + h[i] * scale;
        const double ln = vo + yn[i] - vn;
        v[i] = vn;
        lam[i] = ln;
        en[i] = -(vn - ln - p[i] + q[i]);
        dl = ln - lo;
        dv = vn - vo;
    }
    dl = block_sum256(dl * dl, red);
    dv = block_sum256(dv * dv, red);
    if (threadIdx.x == 0) {
        mpart[blk] = dl;
        mpart[kBpdMaxParts + blk] = dv;
    }
}
__global__ __launch_bounds__(256) void k_bpd_ball(const double* __restrict__ b, const double* __restrict__ h, const double* __restrict__ yn,
                                                  const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ hpart,
                                                  int nparts, double delta, int M, double* __restrict__ v, double* __restrict__ lam,
                                                  double* __restrict__ en, double* __restrict__ mpart) {
    bpd_ball_body((int)blockIdx.x, b, h, yn, p, q, hpart, nparts, delta, M, v, lam, en, mpart);
}

// The group forms of csmp_bpd_batch (host/bpd_batch.hpp), as csmp_bp.hpp's: the member is the grid's third axis, its pointers and its
// ball's radius come from this kernel-argument struct (the live members in entries [0, n), in slot order), its workgroups run the
// single kernels' bodies on the member's own buffers -- per member the arithmetic and the order of every sum are the single solve's.
// k_bpd_ball_group's workgroups read their OWN member's hpart only, written by the launch before: nobody waits, no atomics.
struct BpdGroup {
    int n;
    const double *b[kBpGroupMax], *r[kBpGroupMax];                                 // the member's slot
    double *p[kBpGroupMax], *q[kBpGroupMax], *en[kBpGroupMax], *v[kBpGroupMax], *lam[kBpGroupMax], *h[kBpGroupMax];
    const double* yn[kBpGroupMax];
    double* mpart[kBpGroupMax];                                                    // |lam+ - lam|^2, |v+ - v|^2, |h|^2: kBpdMaxParts each
    double delta[kBpGroupMax];                                                     // the radius of the member's ball
};
static_assert(sizeof(BpdGroup) <= 4096, "kernel arguments");
__global__ __launch_bounds__(256) void k_bpd_pq_group(int M, const BpdGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    bpd_pq_body((int)blockIdx.x, G.b[m], G.r[m], G.en[m], G.yn[m], G.v[m], M, G.p[m], G.q[m], G.h[m], G.mpart[m] + 2 * kBpdMaxParts);
}
__global__ __launch_bounds__(256) void k_bpd_ball_group(int M, int nparts, const BpdGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    bpd_ball_body((int)blockIdx.x, G.b[m], G.h[m], G.yn[m], G.p[m], G.q[m], G.mpart[m] + 2 * kBpdMaxParts, nparts, G.delta[m], M, G.v[m], G.lam[m],
                  G.en[m], G.mpart[m]);
}

// res[0] = |u+ - u|^2, res[1] = |z+ - z|^2 (k_bp_update's partials, k_bp_fold's order), res[2] = |lam+ - lam|^2, res[3] = |v+ - v|^2
// (k_bpd_ball's, eight per thread in index order)
__global__ __launch_bounds__(256) void k_bpd_fold(const double* __restrict__ rpart, int nseg, const double* __restrict__ mpart, int nparts,
                                                  double* __restrict__ res) {
    __shared__ double red[4];
    double s[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 4 * threadIdx.x + k;
            if (j < nseg) a += rpart[h * kIstaMaxSegs + j];
        }
        s[h] = block_sum256(a, red);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < kBpdMaxParts / 256; ++k) {
            const int j = (kBpdMaxParts / 256) * threadIdx.x + k;
            if (j < nparts) a += mpart[h * kBpdMaxParts + j];
        }
        s[2 + h] = block_sum256(a, red);
    }
    if (threadIdx.x == 0) {
        res[0] = s[0];
        res[1] = s[1];
        res[2] = s[2];
        res[3] = s[3];
    }
}

}  // namespace csmp
