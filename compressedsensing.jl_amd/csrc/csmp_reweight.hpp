// csmp_reweight.hpp -- gfx950 kernels of the reweighted l1 path: candes_weights! / ard_weights! (src/basispursuit.jl:33-65) and the
// pieces of the outer loop basispursuit_reweighting (:18-31) runs around ista / fista.
//
// Candes:  w_j = 1 / (|x_j| + eps).
// ARD:     w_j = sqrt(max(a_j' K^-1 a_j, 0)),  K = eps I + A diag(d) A',  d = |x| ./ w,  `iter` times over.  Only d_S, S = supp(x),
//          k = |S|, is non-zero, so with G = A_S'A_S,  H = eps diag(1 / d_S) + G = L L'  (Woodbury)
//              a_j' K^-1 a_j = (|a_j|^2 - |L^-1 A_S' a_j|^2) / eps.
//          Iterations 1 .. iter-1 need w_S only (the next d_S): k x k work, a_i in S has A_S'a_i = G[:, i].  The last one needs all N
//          atoms: the directions W = A_S L^-T (M x k) once, then ONE pass over the dictionary (k_ard_forms).
//   k_rw_support     the support list of x in ascending order, its length, and the checks of x and w (one workgroup: N / 256 trips)
//   k_rw_gather_s    |x_S| and w_S
//   k_rw_gram_sym    G, full and symmetric, from k_gram's row-slice partials (csmp_gram.hpp), added in slice order
//   k_rw_assemble    [H | I] in the layout the blocked Cholesky of csmp_gram.hpp factorises: T = L^-1 comes out beside L'
//   k_rw_inner_w     w_i = sqrt(max((G_ii - |Y[:, i]|^2) / eps, 0)),  Y = T G (k_wgemm)
//   k_rw_dirs        W = A_S T' on the gathered columns
//   k_ard_forms      the N-pass: k_fr_rebuild_lds's scheme (csmp_forward.hpp) over ALL direction blocks, with the column norm and
//                    the epilogue inside
//   k_rw_candes / k_rw_scale / k_rw_stepnorm   the element-wise steps of the outer loop
//
// Determinism: no atomics, no workgroup waits for another, every sum has a fixed order (lane partials in row order, then the
// butterfly; partials of the step norm added on the host in workgroup order): the same bits on every run.
#pragma once
#include "csmp_forward.hpp"
#include "csmp_gram.hpp"
#include "csmp_ista.hpp"

namespace csmp {

constexpr int kRwNormParts = 256;  // workgroups (and partial sums) of k_rw_stepnorm
enum : int { RW_BAD_WEIGHT = 1, RW_BAD_X = 2, RW_BAD_RESULT = 4 };
struct RwInfo {
    int nnz;    // non-zeros of x (all of them, also beyond the list's capacity)
    int flags;  // RW_BAD_*
};

// cols[0 .. min(nnz, cap)) = the indices of the non-zeros of x, ascending.  w (may be NULL): every weight has to be positive and finite.
__global__ __launch_bounds__(256) void k_rw_support(const double* __restrict__ x, const double* __restrict__ w, int64_t N, int cap,
                                                    int* __restrict__ cols, RwInfo* __restrict__ info) {
    __shared__ int wcnt[4];
    __shared__ int sbad[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, bad = 0;
    for (int64_t jt = 0; jt < N; jt += 256) {
        const int64_t j = jt + tid;
        bool nz = false;
        if (j < N) {
            const double xv = x[j];
            nz = xv != 0.0;
            if (!(fabs(xv) < __builtin_inf())) bad |= RW_BAD_X;
            if (w) {
                const double wv = w[j];
                if (!(wv > 0.0) || !(wv < __builtin_inf())) bad |= RW_BAD_WEIGHT;
            }
        }
        const unsigned long long mask = __ballot(nz);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            before += q < wave ? wcnt[q] : 0;
            all += wcnt[q];
        }
        if (nz) {
            const int p = base + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (p < cap) cols[p] = (int)j;
        }
        base += all;
        __syncthreads();
    }
    for (int s = 32; s >= 1; s >>= 1) bad |= __shfl_xor(bad, s, kWave);
    if (lane == 0) sbad[wave] = bad;
    __syncthreads();
    if (tid == 0) {
        info->nnz = base;
        info->flags = sbad[0] | sbad[1] | sbad[2] | sbad[3];
    }
}

__global__ __launch_bounds__(256) void k_rw_gather_s(const double* __restrict__ x, const double* __restrict__ w, const int* __restrict__ cols,
                                                     int k, double* __restrict__ xS, double* __restrict__ wS) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    xS[i] = fabs(x[cols[i]]);
    wS[i] = w[cols[i]];
}

// Gs (np x np, full): entry (row, col) = the sum of k_gram's partials at (min, max) -- the upper tiles are what k_gram computes --;
// zero outside the leading k x k block
__global__ __launch_bounds__(256) void k_rw_gram_sym(const double* __restrict__ Gpart, int nsplit, int k, int np, double* __restrict__ Gs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)np * np) return;
    const int row = (int)(e % np), col = (int)(e / np);
    double s = 0.0;
    if (row < k && col < k) {
        const int64_t u = min(row, col) + (int64_t)max(row, col) * np;
        for (int q = 0; q < nsplit; ++q) s += Gpart[(int64_t)q * np * np + u];
    }
    Gs[e] = s;
}

// Gm (leading dimension npa = 2 np, npa columns): columns [0, np) hold H = G + eps diag(w_S / |x_S|), the identity on the padding
// diagonal; columns [np, np + k) the unit vectors -- the row panels of the factorisation leave T = L^-1 there (csmp_gram.hpp, the
// augmented form of k_gram_reduce).  Rows from np on are never read.
__global__ __launch_bounds__(256) void k_rw_assemble(const double* __restrict__ Gs, const double* __restrict__ xS, const double* __restrict__ wS,
                                                     double eps, int k, int np, int npa, double* __restrict__ Gm) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)npa * npa) return;
    const int row = (int)(e % npa), col = (int)(e / npa);
    if (row >= np) return;
    double v;
    if (col < np) {
        if (row < k && col < k) {
            v = Gs[row + (int64_t)col * np];
            if (row == col) v += eps * wS[row] / xS[row];
        } else {
            v = row == col ? 1.0 : 0.0;
        }
    } else {
        v = (row < k && row == col - np) ? 1.0 : 0.0;
    }
    Gm[e] = v;
}

// w_S of an inner iteration: a_i' K^-1 a_i = (G_ii - sum_t Y[t, i]^2) / eps with Y = L^-1 G; one wave per atom of the support
__global__ __launch_bounds__(256) void k_rw_inner_w(const double* __restrict__ Gs, const double* __restrict__ Y, int k, int np, double eps,
                                                    const DevState* __restrict__ st, double* __restrict__ wS) {
    if (st->done & STOP_REORTH) return;  // (H was not positive definite: the host refuses the call)
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= k) return;
    const double* col = Y + (int64_t)i * np;
    double a0 = 0.0, a1 = 0.0;
    int t = lane;
    for (; t + 64 < k; t += 128) {
        a0 = fma(col[t], col[t], a0);
        a1 = fma(col[t + 64], col[t + 64], a1);
    }
    if (t < k) a0 = fma(col[t], col[t], a0);
    double a = a0 + a1;
    for (int s = 32; s >= 1; s >>= 1) a += shx(a, s);
    if (lane == 0) wS[i] = sqrt(fmax((Gs[i + (int64_t)i * np] - a) / eps, 0.0));
}

// W[m, j] = sum_{i <= j} Ac[m, i] T[j, i]: the directions A_S L^-T on the gathered columns Ac (ldo rows, zero beyond M), T lower
// triangular with leading dimension ldt.  W has ldw >= ldo rows (whole 64-row blocks: k_ard_forms loads them unguarded); the rows
// from ldo on are written as zeros.  32 x 32 output tiles, K-tiles of 32 through the LDS, the next K-tile on its way meanwhile
// (k_wgemm's scheme); K-tiles past the output tile's columns are skipped.
template <typename TA>
__global__ __launch_bounds__(256) void k_rw_dirs(const TA* __restrict__ Ac, int64_t ldo, const double* __restrict__ T, int ldt, int k,
                                                 double* __restrict__ W, int64_t ldw) {
    constexpr int TM = 32, TN = 32, TK = 32;
    __shared__ double As[TK][TM + 1];  // As[i][m] = Ac[m0 + m, i0 + i]
    __shared__ double Bs[TK][TN + 1];  // Bs[i][j] = T[j0 + j, i0 + i]
    const int m0 = blockIdx.x * TM, j0 = blockIdx.y * TN;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int li = threadIdx.x & 31, lk = threadIdx.x >> 5;
    double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;
    const int kend = min(k, j0 + TN);
    double ra[4], rb[4];
    auto fetch = [&](int i0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = i0 + lk + 8 * q;
            const int gm = m0 + li, gj = j0 + li;
            ra[q] = (gm < ldo && gi < k) ? (double)Ac[gm + (int64_t)gi * ldo] : 0.0;
            rb[q] = (gj < k && gi <= gj) ? T[gj + (int64_t)gi * ldt] : 0.0;
        }
    };
    fetch(0);
    for (int i0 = 0; i0 < kend; i0 += TK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            As[lk + 8 * q][li] = ra[q];
            Bs[lk + 8 * q][li] = rb[q];
        }
        __syncthreads();
        if (i0 + TK < kend) fetch(i0 + TK);
#pragma unroll 8
        for (int i = 0; i < TK; ++i) {
            const double a0 = As[i][tx], a1 = As[i][tx + 16], b0 = Bs[i][ty], b1 = Bs[i][ty + 16];
            acc00 = fma(a0, b0, acc00);
            acc01 = fma(a0, b1, acc01);
            acc10 = fma(a1, b0, acc10);
            acc11 = fma(a1, b1, acc11);
        }
        __syncthreads();
    }
    const int gm0 = m0 + tx, gm1 = m0 + tx + 16, gj0 = j0 + ty, gj1 = j0 + ty + 16;
    if (gm0 < ldw && gj0 < k) W[gm0 + (int64_t)gj0 * ldw] = acc00;
    if (gm0 < ldw && gj1 < k) W[gm0 + (int64_t)gj1 * ldw] = acc01;
    if (gm1 < ldw && gj0 < k) W[gm1 + (int64_t)gj0 * ldw] = acc10;
    if (gm1 < ldw && gj1 < k) W[gm1 + (int64_t)gj1 * ldw] = acc11;
}

// The N-pass of ard_weights!: w_j = sqrt(max((|a_j|^2 - sum_d (w_d' a_j)^2) / eps, 0)) for every atom, the k directions w_d the
// columns of W (ldw = whole 64-row blocks, zero rows beyond M).  k_fr_rebuild_lds's scheme -- a workgroup owns 128 atoms (4 waves x
// 2 tiles of 16), a block of 128 directions x 64 rows is staged in the LDS (double-buffered, the next block's loads in flight under
// the current block's 256 MFMAs per wave), v_mfma_f64_16x16x4_f64, the last row block with clamped row indices and masked values
// -- run over ALL ceil(k / 128) direction blocks inside the kernel: the sum of squares stays in registers across the blocks, |a_j|^2
// is taken from the column as it streams past under the first block, and the epilogue writes every w_j exactly once.  The last
// direction block is zero-padded in the LDS; k = 0 runs one all-zero block (w_j = |a_j| / sqrt(eps)).
// fr_rebuild_lds_bytes() of dynamic LDS.  VEC: the columns start on 16-byte boundaries (16-byte non-temporal loads).
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void k_ard_forms(const TA* __restrict__ A, int64_t ld, int M, int64_t N, const double* __restrict__ W,
                                                   int64_t ldw, int k, double eps, double* __restrict__ w) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef TA ta4 __attribute__((ext_vector_type(16 / sizeof(TA))));
    constexpr int NA = 2, NT = kRbDirs / 16, PERV = 16 / (int)sizeof(TA), NV = 16 / PERV;
    extern __shared__ __attribute__((aligned(16))) double rwlds[];
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
    const int nblk = k > 0 ? (k + kRbDirs - 1) / kRbDirs : 1;
    const int total = nblk * nrb;
    d2 stage[16];
    TA raw[NA][16];
    d4 acc[NA][NT];
    double ssum[NA], nrm[NA];
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        ssum[h] = nrm[h] = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
    }

    auto fetch_q = [&](int db, int rb) {  // (a direction past the block's end re-reads the block's first: valid memory, masked in store_q)
        const int nd = k - db * kRbDirs;
        const double* src = W + (int64_t)db * kRbDirs * ldw + (int64_t)rb * kRbRows + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dir = ldir + 8 * j;
            stage[j] = *reinterpret_cast<const d2*>(src + (int64_t)(dir < nd ? dir : 0) * ldw);
        }
    };
    auto store_q = [&](int buf, int db) {
        const int nd = k - db * kRbDirs;
        double* dst = rwlds + (size_t)buf * kRbDirs * kRbStride + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dir = ldir + 8 * j;
            *reinterpret_cast<d2*>(dst + dir * kRbStride) = dir < nd ? stage[j] : d2{0.0, 0.0};
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
        const double* src = rwlds + (size_t)buf * kRbDirs * kRbStride + fq * 16;
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
    store_q(0, 0);
    __syncthreads();
    int buf = 0, db = 0, rb = 0;
    for (int it = 0; it < total; ++it) {
        const bool lastrow = rb + 1 == nrb;
        double bv[NA][16];
        const int r0 = rb * kRbRows + fq * 16;
#pragma unroll
        for (int h = 0; h < NA; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) bv[h][e] = (!lastrow || r0 + e < M) ? (double)raw[h][e] : 0.0;
        if (db == 0) {
#pragma unroll
            for (int h = 0; h < NA; ++h)
#pragma unroll
                for (int e = 0; e < 16; ++e) nrm[h] = fma(bv[h][e], bv[h][e], nrm[h]);
        }
        const int rbn = lastrow ? 0 : rb + 1, dbn = lastrow ? db + 1 : db;
        const bool more = it + 1 < total;
        if (more) {
            fetch_q(dbn, rbn);
            fetch_a(rbn);
        }
        compute(buf, bv);
        if (more) store_q(buf ^ 1, dbn);
        __syncthreads();
        buf ^= 1;
        if (lastrow) {  // a direction block is complete: its squares join the sum, in tile and register order
#pragma unroll
            for (int h = 0; h < NA; ++h)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) ssum[h] = fma(acc[h][t][reg], acc[h][t][reg], ssum[h]);
                    acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
                }
        }
        rb = rbn;
        db = dbn;
    }
    if (a0 >= N) return;
    // C/D layout: column = lane & 15 (the atom), row = (lane >> 4) + 4 reg (the direction): the four lane quarters hold a quarter of
    // the directions -- and of the rows of the norm -- each
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        double s = ssum[h], n2 = nrm[h];
        s += shx(s, 16);
        s += shx(s, 32);
        n2 += shx(n2, 16);
        n2 += shx(n2, 32);
        if (fq == 0 && a0 + h * 16 + fr < N) w[a0 + h * 16 + fr] = sqrt(fmax((n2 - s) / eps, 0.0));
    }
}

// w_j = 1 / (|x_j| + eps) (candes_weight, src/basispursuit.jl:33) and lw_j = lambda w_j, the weights of the next solve
__global__ __launch_bounds__(256) void k_rw_candes(const double* __restrict__ x, int64_t N, double eps, double lambda, double* __restrict__ w,
                                                   double* __restrict__ lw, RwInfo* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double v = 1.0 / (fabs(x[j]) + eps), lv = lambda * v;
    w[j] = v;
    lw[j] = lv;
    if (!(v < __builtin_inf()) || !(lv < __builtin_inf())) info->flags = RW_BAD_RESULT;  // (NaN or Inf, :36; every writer stores the same word)
}
__global__ __launch_bounds__(256) void k_rw_scale(const double* __restrict__ w, int64_t N, double lambda, double* __restrict__ lw,
                                                  RwInfo* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double lv = lambda * w[j];
    lw[j] = lv;
    if (!(lv < __builtin_inf())) info->flags = RW_BAD_RESULT;
}
// the epilogue of the SPLIT form csmp_bench_ard_forms measures (one k_fr_rebuild_lds launch per direction block on rho2 = |a_j|^2)
__global__ __launch_bounds__(256) void k_rw_split_root(const double* __restrict__ rho2, int64_t N, double eps, double* __restrict__ w) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) w[j] = sqrt(fmax(rho2[j] / eps, 0.0));
}
// part[g] = sum of (xs_j - x_j)^2 over workgroup g's contiguous share of the atoms (thread partials in index order, then
// block_sum256); the host adds the kRwNormParts partials in order
__global__ __launch_bounds__(256) void k_rw_stepnorm(const double* __restrict__ xs, const double* __restrict__ x, int64_t N,
                                                     double* __restrict__ part) {
    __shared__ double red[4];
    const int64_t per = ((N + kRwNormParts - 1) / kRwNormParts + 255) / 256 * 256;
    const int64_t j0 = (int64_t)blockIdx.x * per, j1 = j0 + per < N ? j0 + per : N;
    double s = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const double d = xs[j] - x[j];
        s = fma(d, d, s);
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

}  // namespace csmp
