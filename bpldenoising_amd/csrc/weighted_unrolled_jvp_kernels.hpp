// weighted_unrolled_jvp_kernels.hpp -- forward mode through the PDHG iterations of the TV model with a per-pixel data-fidelity
// weight (bpltv_weighted_unrolled_jvp / bpltv_weighted_unrolled_gauss_newton): the weighted solve that
// carries a tangent (dx, dy1, dy2) beside (x, y1, y2) and records nothing.  The exact transpose of the reverse sweep of
// weighted_unrolled_kernels.hpp, with a third tangent dw that the TV sweep (unrolled_jvp_kernels.hpp) does not have; like the
// reverse sweep it needs no w > 0, so a mask (w in {0, 1}) has sensitivities in f, alpha and w.  No tape, 12 state planes
// whatever the iteration count.
//
// Primal = weighted_unrolled_tile_kernel<false>'s, operation for operation, so x after K iterations is
// bpltv_weighted_denoise's u bit for bit (tests/test_gpu_weighted_unrolled_jvp.py).  Tangent of iteration k, per pixel, from
// dx = df, dy = 0 (-ffp-contract=off; no fma in it):
//     ddiv = G^T dy;  r = 1.0 / fma(tau_k, w, 1.0)                    (the primal's own r; x_{k+1} its new iterate)
//     dxn  = (dx - tau_k*((ddiv - w*df) - dw*(f - x_{k+1})))*r
//     dxb  = (1 + omega_k)*dxn - omega_k*dx;  dx = dxn
//     dz   = dy + sigma_k * G dxb
//     n2 = fma(z2, z2, z1*z1);  out = n2 > alpha^2                   (the primal's own expression and decision)
//     out:  q = rsqrt_nr(n2); e = z*q; dot = e1*dz1 + e2*dz2; dy = dalpha*e + (alpha*q)*(dz - e*dot)
//     else: dy = dz
// and du = dx after the last step.  The step table (gamma = min w) is held fixed, as the reverse sweep holds it.
#pragma once
#include <hip/hip_runtime.h>

#include "unrolled_jvp_kernels.hpp"
#include "weighted_unrolled_kernels.hpp"

namespace bpltv {

struct WeightedUnrolledJvpArgs {
    const double* in[6];    // x, y1, y2, dx, dy1, dy2 of the state set read (not read by a first launch)
    double* out[6];
    const double* f;        // the dataset, O planes
    const double* w;        // fidelity weight: one plane (wstride 0) or O planes (wstride M*N)
    const double* df;       // O planes, or nullptr: a zero tangent
    const double* dw;       // planes as w, or nullptr: a zero tangent
    const double* alpha;    // am*an doubles, column major
    const double* dalpha;   // am*an doubles, indexed as alpha, or nullptr: a zero tangent
    const double* tab;      // [maxiter][TAB_STRIDE]; the row's 1/(1 + tau) is not read
    size_t wstride;
    int am, an;
    int it0, nit;
    int M, N;
    int halo;
    int first;              // 1: start from x = f, dx = df, y = dy = 0
    int img0;               // first image of this launch (grid.z = images of the launch chain)
};

// One workgroup per tile, grid (nTi, nTj, images), block 1024: weighted_unrolled_tile_kernel<false> with a second set of LDS
// planes (laid out as sy1 / sy2 / sxb, same zero guards) for the tangent duals and dxb, as unrolled_jvp_tile_kernel.  The
// tangent values are written in front of the same two barriers as the primal ones.  Out-of-image lanes hold zero in every
// value, w and dw included (r = 1 there), and keep it.
__global__ __launch_bounds__(UN_R * UN_R) void weighted_unrolled_jvp_tile_kernel(WeightedUnrolledJvpArgs A) {
    constexpr int RI = UN_R, RJ = UN_R, S1 = RI + 1;
    constexpr int PLANES = RJ * S1 + (RJ + 1) * RI + RJ * RI + RI + 1;   // doubles of one set of planes (pdhg_lds_bytes)
    static_assert(PLANES * sizeof(double) == unrolled_lds_bytes(), "the plane layout is pdhg_lds_bytes'");
    extern __shared__ __attribute__((aligned(16))) unsigned char wun_smem[];
    double* smem = reinterpret_cast<double*>(wun_smem);
    double* sy1 = smem;                              // [RJ][S1]
    double* sy2 = smem + RJ * S1;                    // [RJ+1][RI]
    double* sxb = smem + RJ * S1 + (RJ + 1) * RI;    // [RJ][RI] + RI + 1
    double* sd1 = sy1 + PLANES;                      // the tangent's planes
    double* sd2 = sy2 + PLANES;
    double* sdb = sxb + PLANES;
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
    double x = 0.0, y1 = 0.0, y2 = 0.0, dx = 0.0, dy1 = 0.0, dy2 = 0.0;
    if (!first) {
        x = A.in[0][base + pix];
        y1 = A.in[1][base + pix];
        y2 = A.in[2][base + pix];
        dx = A.in[3][base + pix];
        dy1 = A.in[4][base + pix];
        dy2 = A.in[5][base + pix];
    }
    double f = A.f[base + pix];
    double w = A.w[(size_t)img * A.wstride + pix];
    double df = 0.0, dw = 0.0, dal = 0.0;
    if (A.df) df = A.df[base + pix];
    if (A.dw) dw = A.dw[(size_t)img * A.wstride + pix];
    double al = A.alpha[ai];
    if (A.dalpha) dal = A.dalpha[ai];
    const bool row_word = tid < A.nit * TAB_STRIDE;   // nit <= PDHG_MAX_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * A.it0 + tid];
    const bool in = (oi + li < M) && (oj + lj < N);
    if (first) { x = f; y1 = 0.0; y2 = 0.0; dx = df; dy1 = 0.0; dy2 = 0.0; }
    if (!in) {
        f = 0.0; x = 0.0; y1 = 0.0; y2 = 0.0; al = 0.0; w = 0.0;
        df = 0.0; dx = 0.0; dy1 = 0.0; dy2 = 0.0; dal = 0.0; dw = 0.0;
    }
    sy1[lj * S1 + li + 1] = y1;
    sy2[(lj + 1) * RI + li] = y2;
    sd1[lj * S1 + li + 1] = dy1;
    sd2[(lj + 1) * RI + li] = dy2;
    if (tid < RJ) { sy1[tid * S1] = 0.0; sd1[tid * S1] = 0.0; }
    if (tid < RI) { sy2[tid] = 0.0; sd2[tid] = 0.0; }
    if (tid < RI + 1) { sxb[RI * RJ + tid] = 0.0; sdb[RI * RJ + tid] = 0.0; }
    if (row_word) srow[tid] = row_w;
    __syncthreads();

    const int nit = A.nit;
    // Neumann border: at the last image row / column the "neighbour" is the pixel's own xbar cell (difference +0)
    const int l = lj * RI + li;
    const int n1 = l + (((oi + li) < M - 1) ? 1 : 0);
    const int n2 = l + (((oj + lj) < N - 1) ? RI : 0);
    const int qi = oi + li, qj = oj + lj;
    const bool core = qi >= ci0 && qi < ci1 && qj >= cj0 && qj < cj1;
    const size_t idx = base + qi + (size_t)M * qj;   // used by core pixels only
    // halo rows do not need all the iterations (weighted_unrolled_tile_kernel): a wave owns two adjacent rows; core rows run
    // them all.  Every wave executes two barriers for each of the launch's nit iterations: loop_nit in the first loop, the
    // rest in the second.
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    const double wdf = w * df;   // (the same product in every iteration)
    double tau = srow[0], sigma = srow[1], omega = srow[2], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step and its tangent
        const double y1m = sy1[lj * S1 + li];
        const double y2m = sy2[lj * RI + li];
        const double dy1m = sd1[lj * S1 + li];
        const double dy2m = sd2[lj * RI + li];
        const double div = (y1m - y1) + (y2m - y2);
        const double t = __builtin_fma(-w, f, div);
        const double r = 1.0 / __builtin_fma(tau, w, 1.0);
        const double xo = x;
        const double xn = __builtin_fma(-tau, t, xo) * r;
        const double b = __builtin_fma(-omega, xo, opw * xn);
        x = xn;
        const double ddiv = (dy1m - dy1) + (dy2m - dy2);
        const double dt = (ddiv - wdf) - dw * (f - xn);
        const double dxn = (dx - tau * dt) * r;
        const double db = opw * dxn - omega * dx;
        dx = dxn;
        sxb[l] = b;
        sdb[l] = db;
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], nopw = nrow[4];
        // ---- dual step: y <- proj_{|y_ij| <= alpha_ij}(y + sigma * G xbar), and the projection's derivative
        const double d1 = sxb[n1] - b;
        const double d2 = sxb[n2] - b;
        const double dd1 = sdb[n1] - db;
        const double dd2 = sdb[n2] - db;
        double y1n = __builtin_fma(sigma, d1, y1);
        double y2n = __builtin_fma(sigma, d2, y2);
        double dz1 = dy1 + sigma * dd1;
        double dz2 = dy2 + sigma * dd2;
        const double nn = __builtin_fma(y2n, y2n, y1n * y1n);
        const bool outp = nn > al * al;
        if (outp) {   // a wave whose pixels all lie inside the ball skips the rsqrt
            const double q = rsqrt_nr(nn);
            const double v = al * q;
            const double e1 = y1n * q, e2 = y2n * q;
            const double dot = e1 * dz1 + e2 * dz2;
            dz1 = dal * e1 + v * (dz1 - e1 * dot);
            dz2 = dal * e2 + v * (dz2 - e2 * dot);
            y1n = y1n * v;
            y2n = y2n * v;
        }
        y1 = y1n;
        y2 = y2n;
        dy1 = dz1;
        dy2 = dz2;
        sy1[lj * S1 + li + 1] = y1;
        sy2[(lj + 1) * RI + li] = y2;
        sd1[lj * S1 + li + 1] = dy1;
        sd2[(lj + 1) * RI + li] = dy2;
        tau = ntau; sigma = nsigma; omega = nomega; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    if (core) {
        // write-through stores, as weighted_unrolled_tile_kernel: the next launch reads this state from other XCDs
        __hip_atomic_store(&A.out[0][idx], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[1][idx], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[2][idx], y2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[3][idx], dx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[4][idx], dy1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[5][idx], dy2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace bpltv
