// sumregs_unrolled_kernels.hpp -- reverse mode through the PDHG iterations of the sum-of-regularisers model
// (bpltv_sumregs_unrolled_denoise / bpltv_sumregs_unrolled_vjp): the three-dual solve that records
// the six dual components before every projection, and the sweep that runs the recorded iterations backwards.  Unlike the
// implicit derivative (bpltv_sumregs_vjp: a 13-point system with an active-set threshold) it is the exact derivative of the
// K-step map, needs no factorisation and takes any parameter >= 0.  The reference has no counterpart.
//
// Forward = sr_tile_kernel<32, 32> at rho = 0, operation for operation, so u is bpltv_sumregs_denoise's bit for bit
// (tests/test_gpu_sumregs_unrolled.py); in iteration k it also stores z_k^(r) = y_k^(r) + sigma_k G_r xbar_k, r = forward,
// backward, centred.  Reverse, per pixel, k = K-1 ... 0, from gx = dL/du, gy^(r) = gf = ga^(r) = 0 (-ffp-contract=off; fma
// only where written):
//     for r:  n2 = fma(z2, z2, z1*z1);  out = n2 > a_r^2                 (the forward's expression: the same decision)
//             out:  q = rsqrt_nr(n2); e = z*q; dot = e1*gy1 + e2*gy2; gz = (a_r*q)*(gy - e*dot); ga_r += dot
//             else: gz = gy
//             gz components of a difference the pixel does not have (image border) are set to 0
//     gxb = sigma_k * ((G_f^T gz^f + G_b^T gz^b) + G_c^T gz^c)           (the forward's div stencil and summation order)
//     gxn = gx + (1 + omega_k)*gxb;  h = gxn * (1/(1 + tau_k));  gf += tau_k*h
//     gy^(r) = gz^(r) - tau_k * G_r h;  gx = h - omega_k*gxb             (the forward's three difference stencils)
// and dL/df = gf + gx after the last step (x_0 = f, y_0 = 0).
//
// Tape layout (private): [k][component f1, f2, b1, b2, c1, c2][image][pixel], so a wave's stores and loads run along i.
#pragma once
#include <hip/hip_runtime.h>

#include "pdhg_kernels.hpp"
#include "sumregs_kernels.hpp"

namespace bpltv {

constexpr int SRUN_R = 32;       // region of both kernels: 32 x 32, one pixel per thread
constexpr int SRUN_REV_T = 4;    // most reverse iterations per launch: their taped values sit in registers (6 * 4 doubles)

struct SrUnrolledArgs {
    const double* in[7];   // x, yf1, yf2, yb1, yb2, yc1, yc2
    double* out[7];
    const double* f;       // the dataset, O planes
    const double* alpha;   // one block of 3 slices of am*an doubles (SR_SHARED), or one per image, astride apart (SR_EACH)
    const double* tab;     // [maxiter][TAB_STRIDE], L = sqrt(18)
    double* tape;          // [maxiter][6][O][M*N] (TAPE = false: not read)
    size_t plane;          // O * M*N: doubles of one tape component
    int am, an;
    int it0, nit;
    int tk0;               // tape base iteration: iteration k lives in slot k - tk0 (0: the full tape; a checkpointed sweep's
                           // segment tape starts at its segment's first iteration).  tab stays indexed by k itself
    int M, N;
    int halo;              // 2 * fused iterations
    int first;             // 1: start from x = f, y = 0
    int img0;              // first image of this launch (grid.z = images of the launch chain)
    int astride;           // SR_EACH: doubles per parameter block, 3 * am * an
};

// One workgroup per tile, grid (nTi, nTj, images), block 1024: sr_tile_kernel<32, 32> without the Huber branch, plus six
// stores per iteration -- the duals before their projection -- for the core pixels (valid in every iteration of a launch).
// TAPE = false: the same recurrence without those stores (the checkpoint pass).
template <SrAddr ADDR, bool TAPE = true>
__global__ __launch_bounds__(SRUN_R* SRUN_R) void sr_unrolled_tile_kernel(SrUnrolledArgs A) {
    static_assert(ADDR == SR_SHARED || ADDR == SR_EACH, "the taped solve runs in the dataset context");
    constexpr int RI = SRUN_R, RJ = SRUN_R, RN = RI * RJ;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* sy = smem;              // six planes [RJ][RI]
    double* sxb = smem + 6 * RN;
    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y;
    const int img = A.img0 + (int)blockIdx.z;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, A.M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, A.N, RJ, A.halo, oj, cj0, cj1);
    const int M = A.M, N = A.N;
    const size_t base = (size_t)img * M * N;
    const double* __restrict__ alpha = A.alpha + (ADDR == SR_EACH ? (size_t)img * A.astride : (size_t)0);
    const int gi = oi + li, gj = oj + lj;
    const bool in = gi < M && gj < N;
    const int ci = min(gi, M - 1), cj = min(gj, N - 1);
    const size_t q = ci + (size_t)M * cj, g = base + q;
    const size_t ai = sr_alpha_index(A.am, A.an, M, N, ci, cj), sl = (size_t)A.am * A.an;
    // ---- prologue: all global loads first
    double x, f, y[6], al[3];
    f = A.f[g];
    al[0] = alpha[ai]; al[1] = alpha[sl + ai]; al[2] = alpha[2 * sl + ai];
    if (!A.first) {
        x = A.in[0][g];
#pragma unroll
        for (int c = 0; c < 6; ++c) y[c] = A.in[1 + c][g];
    } else {
        x = f;
#pragma unroll
        for (int c = 0; c < 6; ++c) y[c] = 0.0;
    }
    if (!in) {
        x = 0.0; f = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) y[c] = 0.0;
        al[0] = al[1] = al[2] = 0.0;
    }
    const int l = lj * RI + li;
    // image-border flags, clamped neighbour offsets and the zero cell behind the planes: as sr_tile_kernel
    const bool hasL = gi > 0, hasR = gi < M - 1, hasU = gj > 0, hasD = gj < N - 1;
    const int nim = l - ((hasL && li > 0) ? 1 : 0), nip = l + ((hasR && li < RI - 1) ? 1 : 0);
    const int njm = l - ((hasU && lj > 0) ? RI : 0), njp = l + ((hasD && lj < RJ - 1) ? RI : 0);
    const int zf1m = hasL ? nim : (7 - 0) * RN, zf2m = hasU ? njm : (7 - 1) * RN;
    const int zb1p = hasR ? nip : (7 - 2) * RN, zb2p = hasD ? njp : (7 - 3) * RN;
    if (tid == 0) smem[7 * RN] = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) sy[c * RN + l] = y[c];
    __syncthreads();

    const bool core = gi >= ci0 && gi < ci1 && gj >= cj0 && gj < cj1;
    const size_t idx = base + gi + (size_t)M * gj;   // used by core pixels only
    double* tz = TAPE ? A.tape + (size_t)6 * A.plane * (A.it0 - A.tk0) + idx : nullptr;
    const double* __restrict__ row = A.tab + (size_t)TAB_STRIDE * A.it0;
    double tau = row[0], sigma = row[1], omega = row[2], inv1ptau = row[3], opw = row[4];
    for (int it = 0; it < A.nit; ++it) {
        const double* __restrict__ nrow = row + TAB_STRIDE * ((it + 1 < A.nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], ninv1ptau = nrow[3], nopw = nrow[4];
        // ---- primal step: div = (G_f^T y_f + G_b^T y_b) + G_c^T y_c in the oracle's gather order
        const double f1m = sy[0 * RN + zf1m], f2m = sy[1 * RN + zf2m];
        const double b1p = sy[2 * RN + zb1p], b2p = sy[3 * RN + zb2p];
        const double c1m = sy[4 * RN + nim], c1p = sy[4 * RN + nip];
        const double c2m = sy[5 * RN + njm], c2p = sy[5 * RN + njp];
        const double tf = (f1m - y[0]) + (f2m - y[1]);
        const double tbk = (y[2] - b1p) + (y[3] - b2p);
        const double ca = hasL ? c1m : -y[4], cb = hasR ? c1p : -y[4];
        const double cc = hasU ? c2m : -y[5], cd = hasD ? c2p : -y[5];
        const double tc = 0.5 * (ca - cb) + 0.5 * (cc - cd);
        const double div = (tf + tbk) + tc;
        const double tt = div - f;
        const double xo = x;
        const double xn = __builtin_fma(-tau, tt, xo) * inv1ptau;
        const double bc = __builtin_fma(-omega, xo, opw * xn);
        x = xn;
        sxb[l] = bc;
        __syncthreads();
        // ---- dual steps
        const double bp = sxb[nip], bm = sxb[nim], cp = sxb[njp], cm = sxb[njm];
        double d1[3], d2[3];
        d1[0] = bp - bc; d2[0] = cp - bc;
        d1[1] = bc - bm; d2[1] = bc - cm;
        d1[2] = 0.5 * (bp - bm); d2[2] = 0.5 * (cp - cm);
        double n2v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            y[2 * k] = __builtin_fma(sigma, d1[k], y[2 * k]);
            y[2 * k + 1] = __builtin_fma(sigma, d2[k], y[2 * k + 1]);
            n2v[k] = __builtin_fma(y[2 * k + 1], y[2 * k + 1], y[2 * k] * y[2 * k]);
        }
        if (TAPE) {
            if (core) {   // the tape: the duals before their projection
#pragma unroll
                for (int c = 0; c < 6; ++c) __hip_atomic_store(tz + c * A.plane, y[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            tz += 6 * A.plane;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // per regulariser: lanes outside the ball project
            const double a = al[k];
            if (n2v[k] > a * a) {
                const double v = a * rsqrt_nr(n2v[k]);
                y[2 * k] = y[2 * k] * v;
                y[2 * k + 1] = y[2 * k + 1] * v;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) sy[c * RN + l] = y[c];
        tau = ntau; sigma = nsigma; omega = nomega; inv1ptau = ninv1ptau; opw = nopw;
        __syncthreads();
    }
    if (core) {
        // write-through stores, as sr_tile_kernel: the next launch reads this state from other XCDs
        __hip_atomic_store(&A.out[0][idx], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int c = 0; c < 6; ++c) __hip_atomic_store(&A.out[1 + c][idx], y[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct SrUnrolledRevArgs {
    const double* in[7];   // gx, gyf1, gyf2, gyb1, gyb2, gyc1, gyc2; first: in[0] is the cotangent dL/du, the others are not read
    double* out[7];
    double* gf;            // in place, owning core only
    double* ga;            // in place, owning core only: three planes [3][O][M*N], the per-pixel, per-image parameter gradient
    const double* tape;    // [maxiter][6][O][M*N]
    const double* alpha;
    const double* tab;
    size_t plane;
    int am, an;
    int khi, nit;          // this launch runs the iterations khi, khi - 1, ..., khi - nit + 1
    int tk0;               // tape base iteration, as SrUnrolledArgs (khi - nit + 1 >= tk0)
    int M, N;
    int halo;              // 2 * fused reverse iterations
    int first;             // 1: start from gx = in[0], gy = gf = ga = 0
    int img0;
    int astride;
};

// The mirror image: same region, halo and tile_span, nit <= SRUN_REV_T reverse iterations per launch.  The seven cotangent
// planes ping-pong between two state sets; gf and the three ga planes are read and written by the owning core only.  The six
// gz components go through the six dual planes (G_f^T, G_b^T, G_c^T: the forward's div stencil) and h through the seventh
// (the forward's three difference stencils).  The forward keeps yf1 = +0 where a pixel has no right neighbour in the image
// (yf2: none below, yb1: none to the left, yb2: none above) only because that difference is x - x; here the same holds
// for gz only because it is enforced: those components are set to 0 before they enter the planes.  The centred operator
// (oracle/np_twin_sumregs.diff_matrix: 0.5 * (x[min(i+1, M-1)] - x[max(i-1, 0)])) needs no mask -- its transpose at an
// image border is the forward's `hasL ? c1m : -y` form, taken over as it is.
template <SrAddr ADDR>
__global__ __launch_bounds__(SRUN_R* SRUN_R) void sr_unrolled_reverse_tile_kernel(SrUnrolledRevArgs A) {
    static_assert(ADDR == SR_SHARED || ADDR == SR_EACH, "the reverse sweep runs in the dataset context");
    constexpr int RI = SRUN_R, RJ = SRUN_R, RN = RI * RJ;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* sg = smem;              // six planes [RJ][RI]: gz
    double* sh = smem + 6 * RN;     // h
    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y;
    const int img = A.img0 + (int)blockIdx.z;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, A.M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, A.N, RJ, A.halo, oj, cj0, cj1);
    const int M = A.M, N = A.N;
    const size_t base = (size_t)img * M * N;
    const double* __restrict__ alpha = A.alpha + (ADDR == SR_EACH ? (size_t)img * A.astride : (size_t)0);
    const int gi = oi + li, gj = oj + lj;
    const bool in = gi < M && gj < N;
    const int ci = min(gi, M - 1), cj = min(gj, N - 1);
    const size_t q = ci + (size_t)M * cj, g = base + q;
    const size_t ai = sr_alpha_index(A.am, A.an, M, N, ci, cj), sl = (size_t)A.am * A.an;
    const bool core = gi >= ci0 && gi < ci1 && gj >= cj0 && gj < cj1;
    const bool first = A.first != 0;
    const int nit = A.nit;

    // ---- prologue: every global load, the launch's taped values included, is issued before the first use
    double gx = A.in[0][g], gy[6], gf = 0.0, ga[3] = {0.0, 0.0, 0.0}, al[3];
#pragma unroll
    for (int c = 0; c < 6; ++c) gy[c] = 0.0;
    if (!first) {
#pragma unroll
        for (int c = 0; c < 6; ++c) gy[c] = A.in[1 + c][g];
        if (core) {
            gf = A.gf[g];
#pragma unroll
            for (int r = 0; r < 3; ++r) ga[r] = A.ga[r * A.plane + g];
        }
    }
    al[0] = alpha[ai]; al[1] = alpha[sl + ai]; al[2] = alpha[2 * sl + ai];
    double z[SRUN_REV_T][6];   // [s]: iteration khi - s
    const double* tz = A.tape + (size_t)6 * A.plane * (A.khi - A.tk0) + g;
#pragma unroll
    for (int s = 0; s < SRUN_REV_T; ++s) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            z[s][c] = 0.0;
            if (s < nit) z[s][c] = tz[c * A.plane];
        }
        tz -= 6 * A.plane;
    }
    if (!in) {
        gx = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) gy[c] = 0.0;
        al[0] = al[1] = al[2] = 0.0;
    }
    const int l = lj * RI + li;
    const bool hasL = gi > 0, hasR = gi < M - 1, hasU = gj > 0, hasD = gj < N - 1;
    const int nim = l - ((hasL && li > 0) ? 1 : 0), nip = l + ((hasR && li < RI - 1) ? 1 : 0);
    const int njm = l - ((hasU && lj > 0) ? RI : 0), njp = l + ((hasD && lj < RJ - 1) ? RI : 0);
    const int zf1m = hasL ? nim : (7 - 0) * RN, zf2m = hasU ? njm : (7 - 1) * RN;
    const int zb1p = hasR ? nip : (7 - 2) * RN, zb2p = hasD ? njp : (7 - 3) * RN;
    if (tid == 0) smem[7 * RN] = 0.0;
    // (the first barrier of the loop orders the zero cell before its first read)

#pragma unroll
    for (int s = 0; s < SRUN_REV_T; ++s) {
        if (s < nit) {   // (uniform)
            const double* __restrict__ row = A.tab + (size_t)TAB_STRIDE * (A.khi - s);
            const double tau = row[0], sigma = row[1], omega = row[2], inv1ptau = row[3], opw = row[4];
            // ---- adjoint of the three projections, on the taped duals
            double gz[6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double a = al[r];
                const double za = in ? z[s][2 * r] : 0.0, zb = in ? z[s][2 * r + 1] : 0.0;
                const double nn = __builtin_fma(zb, zb, za * za);
                double g1 = gy[2 * r], g2 = gy[2 * r + 1];
                if (nn > a * a) {
                    const double qq = rsqrt_nr(nn);
                    const double u1 = za * qq, u2 = zb * qq;
                    const double dot = u1 * g1 + u2 * g2;
                    const double v = a * qq;
                    g1 = v * (g1 - u1 * dot);
                    g2 = v * (g2 - u2 * dot);
                    ga[r] += dot;
                }
                gz[2 * r] = g1;
                gz[2 * r + 1] = g2;
            }
            // the differences this pixel does not have
            gz[0] = hasR ? gz[0] : 0.0; gz[1] = hasD ? gz[1] : 0.0;
            gz[2] = hasL ? gz[2] : 0.0; gz[3] = hasU ? gz[3] : 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) sg[c * RN + l] = gz[c];
            __syncthreads();
            // ---- adjoint of the dual step's differences (the forward's div), of the over-relaxation and of the primal step
            const double f1m = sg[0 * RN + zf1m], f2m = sg[1 * RN + zf2m];
            const double b1p = sg[2 * RN + zb1p], b2p = sg[3 * RN + zb2p];
            const double c1m = sg[4 * RN + nim], c1p = sg[4 * RN + nip];
            const double c2m = sg[5 * RN + njm], c2p = sg[5 * RN + njp];
            const double tf = (f1m - gz[0]) + (f2m - gz[1]);
            const double tbk = (gz[2] - b1p) + (gz[3] - b2p);
            const double ca = hasL ? c1m : -gz[4], cb = hasR ? c1p : -gz[4];
            const double cc = hasU ? c2m : -gz[5], cd = hasD ? c2p : -gz[5];
            const double tc = 0.5 * (ca - cb) + 0.5 * (cc - cd);
            const double gxb = sigma * ((tf + tbk) + tc);
            const double gxn = gx + opw * gxb;
            const double h = gxn * inv1ptau;
            sh[l] = h;
            __syncthreads();
            const double bp = sh[nip], bm = sh[nim], cp = sh[njp], cm = sh[njm];
            gf += tau * h;
            gy[0] = gz[0] - tau * (bp - h); gy[1] = gz[1] - tau * (cp - h);
            gy[2] = gz[2] - tau * (h - bm); gy[3] = gz[3] - tau * (h - cm);
            gy[4] = gz[4] - tau * (0.5 * (bp - bm)); gy[5] = gz[5] - tau * (0.5 * (cp - cm));
            gx = h - omega * gxb;
        }
    }

    if (core) {
        const size_t idx = base + gi + (size_t)M * gj;
        __hip_atomic_store(&A.out[0][idx], gx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int c = 0; c < 6; ++c) __hip_atomic_store(&A.out[1 + c][idx], gy[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.gf[idx], gf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int r = 0; r < 3; ++r) __hip_atomic_store(&A.ga[r * A.plane + idx], ga[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace bpltv
