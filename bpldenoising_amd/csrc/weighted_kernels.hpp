// weighted_kernels.hpp -- the TV model with a per-pixel data-fidelity weight,
//     min_u 0.5 sum w_ij (u_ij - f_ij)^2 + sum alpha_ij |(G u)_ij|,      w >= 0,
// (bpltv_weighted_denoise / bpltv_weighted_vjp): the fused PDHG kernel, its duality gap, and the
// setup and output kernels of its adjoint.  The reference has no counterpart: its denoise fixes the fidelity at one
// (/root/reference/src/TVLearningFunctionVec.jl:45-70).
//
// Recurrence = "spec v2" of pdhg_tile_kernel with three operations changed (per pixel, explicit fma, -ffp-contract=off):
//     t     = fma(-w, f, div)                  (div - f there)
//     r     = 1.0 / fma(tau, w, 1.0)           (IEEE division; the tabulated 1/(1 + tau) there)
//     x_new = fma(-tau, t, x) * r
// and the step table built with gamma = min w instead of 1.  With w == 1.0 each of them returns the bits of the
// operation it replaces, so the result is bpltv_denoise's bit for bit (tests/test_gpu_weighted.py).
#pragma once
#include <hip/hip_runtime.h>

#include "adjoint_kernels.hpp"
#include "pdhg_kernels.hpp"

namespace bpltv {

constexpr int WT_R = 32;   // region (core + halo) of one workgroup: 32 x 32 pixels, one per thread
constexpr size_t weighted_lds_bytes() { return pdhg_lds_bytes(WT_R, WT_R); }   // the dynamic planes; the step rows are static

struct WeightedArgs {
    const double* xin;
    const double* y1in;
    const double* y2in;
    double* xout;
    double* y1out;
    double* y2out;
    const double* f;      // the dataset, O planes
    const double* w;      // fidelity weight: one plane (wstride 0) or O planes (wstride M*N)
    const double* alpha;  // am*an doubles, column major
    const double* tab;    // [maxiter][TAB_STRIDE]; the row's 1/(1 + tau) is not read
    size_t wstride;
    int am, an;
    int it0, nit;
    int M, N;
    int halo;
    int first;            // 1: start from x = f, y = 0
    int img0;             // first image of this launch (grid.z = images of the launch chain)
};

// One workgroup per tile, grid (nTi, nTj, images), block 1024.  pdhg_tile_kernel<double, 1, 1, 32, 32>'s structure: state,
// f, w and alpha in registers for the whole launch, neighbour values through three LDS planes (y1 with a zero guard
// column, y2 with a zero guard row, xbar with pad cells), two barriers per iteration, the launch's step rows in LDS, the
// core written back, halo waves that are past their use keep the barriers company only.
__global__ __launch_bounds__(WT_R * WT_R) void weighted_tile_kernel(WeightedArgs A) {
    constexpr int RI = WT_R, RJ = WT_R, S1 = RI + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_smem[];
    double* smem = reinterpret_cast<double*>(wt_smem);
    double* sy1 = smem;                              // [RJ][S1]
    double* sy2 = smem + RJ * S1;                    // [RJ+1][RI]
    double* sxb = smem + RJ * S1 + (RJ + 1) * RI;    // [RJ][RI] + RI + 1
    __shared__ __attribute__((aligned(16))) double srow[PDHG_MAX_T * TAB_STRIDE];

    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y, img = A.img0 + (int)blockIdx.z;
    const int M = A.M, N = A.N;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, N, RJ, A.halo, oj, cj0, cj1);
    const size_t base = (size_t)img * M * N;
    const int amode = (A.am == 1 && A.an == 1) ? 0 : ((A.am == M && A.an == N) ? 2 : 1);
    const bool first = A.first != 0;

    // ---- prologue: every global load is issued before the first use.  Out-of-image pixels read a clamped in-image
    // address and are zeroed afterwards (w = 0 there: r = 1, the pixel stays 0).
    const int gi = min(oi + li, M - 1), gj = min(oj + lj, N - 1);
    const size_t pix = gi + (size_t)M * gj;
    size_t ai = 0;
    if (amode == 2) {
        ai = pix;
    } else if (amode == 1) {
        const unsigned pa = ((unsigned)gi * (unsigned)A.am) / (unsigned)M;
        const unsigned pb = ((unsigned)gj * (unsigned)A.an) / (unsigned)N;
        ai = pa + (size_t)A.am * pb;
    }
    double x = 0.0, y1 = 0.0, y2 = 0.0;
    if (!first) {
        x = A.xin[base + pix];
        y1 = A.y1in[base + pix];
        y2 = A.y2in[base + pix];
    }
    double f = A.f[base + pix];
    double w = A.w[(size_t)img * A.wstride + pix];
    double al = A.alpha[ai];
    const bool row_word = tid < A.nit * TAB_STRIDE;   // nit <= PDHG_MAX_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * A.it0 + tid];
    const bool in = (oi + li < M) && (oj + lj < N);
    if (first) { x = f; y1 = 0.0; y2 = 0.0; }
    if (!in) { f = 0.0; x = 0.0; y1 = 0.0; y2 = 0.0; al = 0.0; w = 0.0; }
    sy1[lj * S1 + li + 1] = y1;
    sy2[(lj + 1) * RI + li] = y2;
    if (tid < RJ) sy1[tid * S1] = 0.0;
    if (tid < RI) sy2[tid] = 0.0;
    if (tid < RI + 1) sxb[RI * RJ + tid] = 0.0;
    if (row_word) srow[tid] = row_w;
    __syncthreads();

    const int nit = A.nit;
    // Neumann border: at the last image row / column the "neighbour" is the pixel's own xbar cell (difference +0)
    const int l = lj * RI + li;
    const int n1 = l + (((oi + li) < M - 1) ? 1 : 0);
    const int n2 = l + (((oj + lj) < N - 1) ? RI : 0);
    // halo rows do not need all the iterations (pdhg_tile_kernel): a wave owns two adjacent rows
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    double tau = srow[0], sigma = srow[1], omega = srow[2], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step: x <- prox_{tau * fidelity}(x - tau * G^T y); over-relaxation
        const double y1m = sy1[lj * S1 + li];
        const double y2m = sy2[lj * RI + li];
        const double div = (y1m - y1) + (y2m - y2);
        const double t = __builtin_fma(-w, f, div);
        const double r = 1.0 / __builtin_fma(tau, w, 1.0);
        const double xo = x;
        const double xn = __builtin_fma(-tau, t, xo) * r;
        const double b = __builtin_fma(-omega, xo, opw * xn);
        x = xn;
        sxb[l] = b;
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], nopw = nrow[4];
        // ---- dual step: y <- proj_{|y_ij| <= alpha_ij}(y + sigma * G xbar)
        const double d1 = sxb[n1] - b;
        const double d2 = sxb[n2] - b;
        double y1n = __builtin_fma(sigma, d1, y1);
        double y2n = __builtin_fma(sigma, d2, y2);
        const double nn = __builtin_fma(y2n, y2n, y1n * y1n);
        const bool outp = nn > al * al;
        if (outp) {   // a wave whose pixels all lie inside the ball skips the rsqrt
            const double v = al * rsqrt_nr(nn);
            y1n = y1n * v;
            y2n = y2n * v;
        }
        y1 = y1n;
        y2 = y2n;
        sy1[lj * S1 + li + 1] = y1;
        sy2[(lj + 1) * RI + li] = y2;
        tau = ntau; sigma = nsigma; omega = nomega; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    const int qi = oi + li, qj = oj + lj;
    if (qi >= ci0 && qi < ci1 && qj >= cj0 && qj < cj1) {
        const size_t idx = base + qi + (size_t)M * qj;
        // write-through stores, as pdhg_tile_kernel: the next launch reads this state from other XCDs
        __hip_atomic_store(&A.xout[idx], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.y1out[idx], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.y2out[idx], y2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Primal-dual gap pieces per image of the weighted model (gamma = min w > 0), with d = G^T y:
//     partial[(k*nblk+b)*4 + {0: sum w (u-f)^2, 1: sum alpha |G u|, 2: sum d f, 3: sum d^2 / w}]
//     gap = 0.5 s0 + s1 - (s2 - 0.5 s3)  >=  0.5 sum w (u - u*)^2.
// grid (nblk, O), block 256; gap_partial_kernel's sum order, no atomics.
__global__ __launch_bounds__(256) void weighted_gap_partial_kernel(const double* __restrict__ u, const double* __restrict__ y1,
                                                                   const double* __restrict__ y2, const double* __restrict__ f,
                                                                   const double* __restrict__ w, size_t wstride,
                                                                   const double* __restrict__ alpha, int am, int an, int M, int N,
                                                                   double* __restrict__ partial) {
    __shared__ double sh[4];
    const int npx = M * N;
    const size_t base = (size_t)blockIdx.y * npx;
    w += (size_t)blockIdx.y * wstride;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < npx; q += gridDim.x * 256) {
        const int i = q % M, j = q / M;
        const double uk = u[base + q], fk = f[base + q], wk = w[q];
        const double d1 = (i < M - 1) ? u[base + q + 1] - uk : 0.0;
        const double d2 = (j < N - 1) ? u[base + q + M] - uk : 0.0;
        const double a1 = (i < M - 1) ? y1[base + q] : 0.0, a1m = (i > 0) ? y1[base + q - 1] : 0.0;
        const double a2 = (j < N - 1) ? y2[base + q] : 0.0, a2m = (j > 0) ? y2[base + q - M] : 0.0;
        const double d = (a1m - a1) + (a2m - a2);
        const double r = uk - fk;
        s0 += wk * (r * r);
        s1 += alpha_at(alpha, am, an, M, N, i, j) * sqrt(d1 * d1 + d2 * d2);
        s2 += d * fk;
        s3 += d * d / wk;
    }
    s0 = block_sum<256>(s0, sh);
    s1 = block_sum<256>(s1, sh);
    s2 = block_sum<256>(s2, sh);
    s3 = block_sum<256>(s3, sh);
    if (threadIdx.x == 0) {
        double* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3;
    }
}

__global__ __launch_bounds__(256) void weighted_gap_final_kernel(const double* __restrict__ partial, int nblk, int O,
                                                                 double* __restrict__ gap, double* __restrict__ gap_max) {
    for (int k = threadIdx.x; k < O; k += 256) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < nblk; ++b)
            for (int c = 0; c < 4; ++c) s[c] += partial[((size_t)k * nblk + b) * 4 + c];
        gap[k] = (0.5 * s[0] + s[1]) - (s[2] - 0.5 * s[3]);
    }
    __syncthreads();
    if (threadIdx.x == 0 && gap_max) {
        double m = gap[0];
        for (int k = 1; k < O; ++k) m = (gap[k] > m) ? gap[k] : m;
        gap_max[0] = m;
    }
}

// Adjoint of the weighted model (reg = 0: the reference's `gradient` linearisation): the system is diag(w) + K, and with
// S = diag(w)^-1/2 it is S^-1 (I + S K S) S^-1 -- the node-scaled form adj_assemble_kernel, adj_residual_kernel,
// adj_gradpix_kernel and every factorisation handle through the s plane.  adj_setup_body<true> with reg = 0, then
//     s = 1 / sqrt(w),   rhs = gu * s            (w == 1: s = 1 and rhs = gu exactly)
// so that q solves (I + S K S) q = S gu and the physical adjoint state is p = S q.
constexpr double WEIGHTED_KAPPA_CAP = 4e14;
__global__ __launch_bounds__(256) void weighted_adj_setup_kernel(const double* __restrict__ u, const double* __restrict__ gu,
                                                                 const double* __restrict__ w, size_t wstride,
                                                                 const double* __restrict__ alpha, int am, int an, int M, int N,
                                                                 int O, double kappa_act, AdjCoef C) {
    adj_setup_body<true>(u, gu, alpha, am, an, 0, M, N, O, 0, 0, kappa_act, C);
    const size_t npx = (size_t)M * N;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= npx * O) return;
    const double* wp = w + (q / npx) * wstride;
    const int k = (int)(q % npx);
    const double s = 1.0 / sqrt(wp[k]);
    C.s[q] = s;
    C.rhs[q] = gu[q] * s;
    // An active element enters the scaled matrix as kappa s_a s_b.  Above WEIGHTED_KAPPA_CAP (w < 1/4 at kappa = 1e14) those
    // entries pass 1/eps and what ties a flat region to the rest of the image -- the identity and its inactive neighbours --
    // falls below their rounding: every factorisation is then wrong by O(1) in the mode that moves the region as a whole and
    // the refinement stalls or diverges.  So the element's weight is kappa relative to the smallest
    // fidelity weight of its nodes: min(kappa, cap * w_min), which keeps kappa s^2 <= cap on all three.
    const double kp = C.kap[q];
    if (kp > 0.0) {
        const int i = k % M, j = k / M;
        double wmin = wp[k];
        if (i < M - 1) wmin = fmin(wmin, wp[k + 1]);
        if (j < N - 1) wmin = fmin(wmin, wp[k + M]);
        C.kap[q] = fmin(kp, WEIGHTED_KAPPA_CAP * wmin);
    }
}

// The outputs: grad_f = w o p and the per-pixel grad_w = -(u - f) o p, p = s q (adj_gradf_kernel's product).  Either
// pointer may be null; f is read only for grad_w.
__global__ __launch_bounds__(256) void weighted_adj_out_kernel(const double* __restrict__ s, const double* __restrict__ qv,
                                                               const double* __restrict__ w, size_t wstride,
                                                               const double* __restrict__ u, const double* __restrict__ f,
                                                               size_t npx, size_t n, double* __restrict__ grad_f,
                                                               double* __restrict__ grad_w) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const double p = s[q] * qv[q];
    if (grad_f) grad_f[q] = w[(q / npx) * wstride + q % npx] * p;
    if (grad_w) grad_w[q] = -(u[q] - f[q]) * p;
}

}  // namespace bpltv
