// weighted_kernels.hpp -- the TV model with a per-pixel data-fidelity weight,
//     min_u 0.5 sum w_ij (u_ij - f_ij)^2 + sum alpha_ij |(G u)_ij|,      w >= 0,
// (bpltv_weighted_denoise / bpltv_weighted_vjp): its duality gap, and the setup and output kernels of
// its adjoint.  The fused PDHG kernel is tv_tile_kernel<true, false, false> (tv_tile_kernels.hpp, where the recurrence is
// written down).  The reference has no counterpart: its denoise fixes the fidelity at one
// (/root/reference/src/TVLearningFunctionVec.jl:45-70).
#pragma once
#include <hip/hip_runtime.h>

#include "adjoint_kernels.hpp"
#include "pdhg_kernels.hpp"

namespace bpltv {

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
