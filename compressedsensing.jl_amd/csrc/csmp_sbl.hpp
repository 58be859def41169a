// csmp_sbl.hpp -- gfx950 kernels of sparse Bayesian learning, sbl(A, b, sigma2) / update!(::SBL) (src/sbl.jl:1-51), in the Woodbury
// form (include/csmp.h, csmp_sbl).  With Gamma = diag(gam), C = sigma2 I + A Gamma A' = L L' (M x M), for every atom j
//     s_j = |L^-1 a_j|^2,   q_j = (L^-1 a_j)' (L^-1 b),   x_j = gam_j q_j,   gam_j+ = gam_j q_j^2 / s_j + 1e-14
//   k_rowgram<.., WT = true>   (csmp_bp.hpp) sum_c gam_c a_c a_c' on the Float64 matrix cores, one operand scaled as it is staged;
//                      k_rowgram_reduce then gives the symmetric matrix
//   k_sbl_assemble     [C | I], sigma2 added on the diagonal, in the layout the blocked Cholesky of csmp_gram.hpp factorises (k_bp_assemble's)
//   k_sbl_forms        the N-pass: k_ard_forms's scheme (csmp_reweight.hpp) over the M columns of W = L^-T, upper triangular -- the row
//                      blocks below a direction block's triangle are neither loaded nor multiplied -- with s and q from the same projections
//   k_sbl_update       x, gam+, the partials of |gam+ - gam|^2 and the verdict on gam+, element-wise over the N atoms
//   k_sbl_fold         the partials added in workgroup order
//   k_sbl_check / k_sbl_loadb   the checks of a gam handed over in device memory; b as doubles
//
// Determinism: no atomics, no workgroup waits for another, every sum has a fixed order: the same bits on every run.
#pragma once
#include "csmp_bp.hpp"
#include "csmp_reweight.hpp"

namespace csmp {

constexpr int kSblParts = 256;        // workgroups (and partial sums) of k_sbl_update
constexpr double kSblFloor = 1e-14;   // added to every gam+ (src/sbl.jl:33)
struct SblInfo {
    double dg2;     // |gam+ - gam|^2 of the last update
    int bad_gamma;  // 1: an update gave a gam+ that is negative or not finite
    int bad_input;  // 1: the gam handed over holds an entry that is not positive and finite
};

// Gm (leading dimension npa = 2 np, rows [0, np)): columns [0, np) hold C = G + sigma2 I, the identity on the padding diagonal; columns
// [np, np + M) the unit vectors -- k_bp_assemble's layout and pivot rule: pivref[i] = 2 thr C_ii.
__global__ __launch_bounds__(256) void k_sbl_assemble(const double* __restrict__ G, double sigma2, int M, int np, int npa, double thr,
                                                      double* __restrict__ Gm, double* __restrict__ pivref) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)npa * npa) return;
    const int row = (int)(e % npa), col = (int)(e / npa);
    if (row >= np) return;
    double v;
    if (col < np) {
        if (row < M && col < M) {
            v = G[row + (int64_t)col * M];
            if (row == col) v += sigma2;
        } else {
            v = row == col ? 1.0 : 0.0;
        }
        if (row == col) pivref[row] = row < M ? 2.0 * thr * v : 0.0;
    } else {
        v = (row < M && row == col - np) ? 1.0 : 0.0;
    }
    Gm[e] = v;
}

// The N-pass of the update: for every atom j,  s_j = sum_d p_d^2  and  q_j = sum_d p_d t_d  with  p_d = w_d' a_j,  the M directions w_d
// the columns of W (leading dimension ldw, whole 64-row blocks) and tv the M-vector t followed by zeros up to whole blocks of 128.
// W is UPPER TRIANGULAR: of column d only the rows 0 .. d are used.  k_ard_forms's scheme -- a workgroup owns 128 atoms (4 waves x 2 tiles of 16), a block of 128 directions x 64 rows is
// staged in the LDS (double-buffered, the next block's loads in flight under the current block's MFMAs), v_mfma_f64_16x16x4_f64, the
// last row block of A with clamped row indices and masked values -- over all ceil(M / 128) direction blocks.  Direction block D
// (columns 128 D ..) is structurally zero in the rows from 128 (D + 1) on: it runs the row blocks 0 .. min(nrb, 2 (D + 1)) - 1 only, the
// others are never read.  Inside the row blocks it does run, an entry below the diagonal is staged as zero whatever the memory holds
// (k_bp_transpose writes the triangle only).  When a direction block is complete its 128 projections join both sums in tile and
// register order; every s_j and q_j is written exactly once.  fr_rebuild_lds_bytes() of dynamic LDS.  VEC: the columns of A start on
// 16-byte boundaries (16-byte non-temporal loads).
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void k_sbl_forms(const TA* __restrict__ A, int64_t ld, int M, int64_t N, const double* __restrict__ W,
                                                   int64_t ldw, const double* __restrict__ tv, double* __restrict__ s_out,
                                                   double* __restrict__ q_out) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef TA ta4 __attribute__((ext_vector_type(16 / sizeof(TA))));
    constexpr int NA = 2, NT = kRbDirs / 16, PERV = 16 / (int)sizeof(TA), NV = 16 / PERV;
    extern __shared__ __attribute__((aligned(16))) double sblds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t a0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * NA);
    const TA* acol[NA];
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        const int64_t atom = a0 + h * 16 + fr < N ? a0 + h * 16 + fr : N - 1;
        acol[h] = A + atom * ld + fq * 16;
    }
    // loader: thread -> row pair tid % 32 of direction tid / 32 + 8 j (32 threads cover the 512 contiguous bytes of a direction)
    const int lrp = tid & 31, ldir = tid >> 5;
    const int nrb = (M + kRbRows - 1) / kRbRows;
    const int nblk = (M + kRbDirs - 1) / kRbDirs;
    auto rbend = [&](int db) { return min(nrb, 2 * (db + 1)); };  // row blocks direction block db runs
    d2 stage[16];
    TA raw[NA][16];
    d4 acc[NA][NT];
    double ssum[NA], qsum[NA];
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        ssum[h] = qsum[h] = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
    }

    auto fetch_q = [&](int db, int rb) {  // (a direction past the block's end re-reads the block's first: valid memory, masked in store_q)
        const int nd = M - db * kRbDirs;
        const double* src = W + (int64_t)db * kRbDirs * ldw + (int64_t)rb * kRbRows + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dir = ldir + 8 * j;
            stage[j] = *reinterpret_cast<const d2*>(src + (int64_t)(dir < nd ? dir : 0) * ldw);
        }
    };
    auto store_q = [&](int buf, int db, int rb) {
        const int nd = M - db * kRbDirs;
        const int row = rb * kRbRows + lrp * 2;
        double* dst = sblds + (size_t)buf * kRbDirs * kRbStride + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dir = ldir + 8 * j, d = db * kRbDirs + dir;
            d2 v;
            v[0] = (dir < nd && row <= d) ? stage[j][0] : 0.0;
            v[1] = (dir < nd && row + 1 <= d) ? stage[j][1] : 0.0;
            *reinterpret_cast<d2*>(dst + dir * kRbStride) = v;
        }
    };
    auto fetch_a = [&](int rb) {
        if (rb + 1 < nrb) {  // every row of the block exists
#pragma unroll
            for (int h = 0; h < NA; ++h) {
                if (VEC) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const ta4 x = __builtin_nontemporal_load(reinterpret_cast<const ta4*>(acol[h] + (int64_t)rb * kRbRows) + v);
#pragma unroll
                        for (int c = 0; c < PERV; ++c) raw[h][v * PERV + c] = x[c];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) raw[h][e] = acol[h][(int64_t)rb * kRbRows + e];
                }
            }
        } else {  // the last row block: row indices clamped into the column, the values masked below
            const int r0 = rb * kRbRows + fq * 16;
#pragma unroll
            for (int h = 0; h < NA; ++h)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = r0 + e < M ? r0 + e : M - 1;
                    raw[h][e] = acol[h][row - fq * 16];
                }
        }
    };
    auto compute = [&](int buf, const double (&bv)[NA][16]) {
        const double* src = sblds + (size_t)buf * kRbDirs * kRbStride + fq * 16;
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

    fetch_q(0, 0);
    fetch_a(0);
    store_q(0, 0, 0);
    __syncthreads();
    int buf = 0, db = 0, rb = 0;
    while (db < nblk) {
        const bool ragged = rb + 1 == nrb;          // the row block that holds A's last rows
        const bool lastrow = rb + 1 == rbend(db);   // the last row block this direction block runs
        double bv[NA][16];
        const int r0 = rb * kRbRows + fq * 16;
#pragma unroll
        for (int h = 0; h < NA; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) bv[h][e] = (!ragged || r0 + e < M) ? (double)raw[h][e] : 0.0;
        const int rbn = lastrow ? 0 : rb + 1, dbn = lastrow ? db + 1 : db;
        const bool more = dbn < nblk;
        if (more) {
            fetch_q(dbn, rbn);
            fetch_a(rbn);
        }
        compute(buf, bv);
        if (more) store_q(buf ^ 1, dbn, rbn);
        __syncthreads();
        buf ^= 1;
        if (lastrow) {  // a direction block is complete: its projections join the two sums, in tile and register order
            // C/D layout: column = lane & 15 (the atom), row = (lane >> 4) + 4 reg (the direction)
            const double* tb = tv + db * kRbDirs + fq;  // (t is zero from M up to whole direction blocks, as the projections are)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const double td = tb[t * 16 + 4 * reg];
#pragma unroll
                    for (int h = 0; h < NA; ++h) {
                        const double p = acc[h][t][reg];
                        ssum[h] = fma(p, p, ssum[h]);
                        qsum[h] = fma(p, td, qsum[h]);
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < NA; ++h)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
        }
        rb = rbn;
        db = dbn;
    }
    if (a0 >= N) return;
    // the four lane quarters hold a quarter of the directions each
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        double s = ssum[h], q = qsum[h];
        s += shx(s, 16);
        s += shx(s, 32);
        q += shx(q, 16);
        q += shx(q, 32);
        if (fq == 0 && a0 + h * 16 + fr < N) {
            s_out[a0 + h * 16 + fr] = s;
            q_out[a0 + h * 16 + fr] = q;
        }
    }
}

// x_j = gam_j q_j;  gam_j+ = gam_j q_j^2 / s_j + 1e-14 (update!(::SBL), src/sbl.jl:26-35).  s_j = 0 -- a zero column, whose q_j is 0 too
// -- gives x_j = 0 and gam_j+ = 1e-14.  part[g] = the sum of (gam_j+ - gam_j)^2 over workgroup g's contiguous share of the atoms (thread
// partials in index order, then block_sum256).  A gam+ that is negative or not finite sets info->bad_gamma (every writer stores the
// same word).
__global__ __launch_bounds__(256) void k_sbl_update(const double* __restrict__ s, const double* __restrict__ q, int64_t N, double* __restrict__ gam,
                                                    double* __restrict__ x, double* __restrict__ part, SblInfo* __restrict__ info) {
    __shared__ double red[4];
    const int64_t per = ((N + kSblParts - 1) / kSblParts + 255) / 256 * 256;
    const int64_t j0 = (int64_t)blockIdx.x * per, j1 = j0 + per < N ? j0 + per : N;
    double acc = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const double g = gam[j], sj = s[j], qj = q[j];
        double xn = 0.0, gn = kSblFloor;
        if (sj != 0.0) {
            xn = g * qj;
            gn = g * qj * qj / sj + kSblFloor;
        }
        x[j] = xn;
        gam[j] = gn;
        const double d = gn - g;
        acc = fma(d, d, acc);
        if (!(gn >= 0.0) || !(gn < __builtin_inf())) info->bad_gamma = 1;
    }
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// info->dg2 = the kSblParts partials, one per thread, through block_sum256
__global__ __launch_bounds__(256) void k_sbl_fold(const double* __restrict__ part, SblInfo* __restrict__ info) {
    __shared__ double red[4];
    static_assert(kSblParts == 256, "one partial per thread");
    const double v = block_sum256(part[threadIdx.x], red);
    if (threadIdx.x == 0) info->dg2 = v;
}

// a gam handed over in device memory: every entry has to be positive and finite (info->bad_input)
__global__ __launch_bounds__(256) void k_sbl_check(const double* __restrict__ gam, int64_t N, SblInfo* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double g = gam[j];
    if (!(g > 0.0) || !(g < __builtin_inf())) info->bad_input = 1;
}
__global__ __launch_bounds__(256) void k_sbl_ones(double* __restrict__ gam, int64_t N) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) gam[j] = 1.0;
}
template <typename TB>
__global__ __launch_bounds__(256) void k_sbl_loadb(const TB* __restrict__ src, int M, double* __restrict__ b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) b[i] = (double)src[i];
}

}  // namespace csmp
