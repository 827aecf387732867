// tv_tile_kernels.hpp -- the two-dual TV recurrence on a 32 x 32 region: one forward kernel, one reverse kernel, and the flags
// that select what each entry point needs of them.  The reference has no counterpart to any of it: its denoise fixes the
// fidelity at one (/root/reference/src/TVLearningFunctionVec.jl:45-70) and its gradients (:98-135) differentiate the exact
// minimiser, not the iteration.
//
//     tv_tile_kernel<WEIGHTED, TAPE, TANGENT>
//         <1,0,0>  bpltv_weighted_denoise, and the checkpoint pass of the weighted taped solve (4.10)
//         <0,1,0>  bpltv_unrolled_denoise (4.6)                    <0,0,0>  its checkpoint pass (4.10)
//         <1,1,0>  bpltv_weighted_unrolled_denoise (4.8)
//         <0,0,1>  bpltv_unrolled_jvp (4.7)                        <1,0,1>  bpltv_weighted_unrolled_jvp (4.11)
//         <1,1,0,L1>  bpltv_lone_unrolled_denoise (4.18)             <1,0,0,L1>  bpltv_lone_denoise and the checkpoint pass (4.18)
//         <1,1,0,0,KL>  bpltv_kl_unrolled_denoise (4.19)            <1,0,0,0,KL>  bpltv_kl_denoise and the checkpoint pass (4.19)
//         <1,0,1,L1>  bpltv_lone_unrolled_jvp (4.20)                 <1,0,1,0,KL>  bpltv_kl_unrolled_jvp (4.20)
//     tv_reverse_tile_kernel<WEIGHTED, L1, KL>
//         <0>      bpltv_unrolled_vjp (4.6)                        <1>      bpltv_weighted_unrolled_vjp (4.8)
//         <1,L1>   bpltv_lone_unrolled_vjp (4.18)                  <1,0,KL> bpltv_kl_unrolled_vjp (4.19)
//
// Forward, per pixel, iteration k = 0 ... K-1 from x = f, y = 0 ("spec v2" of pdhg_tile_kernel<double, 1, 1, 32, 32> with
// rho = 0; explicit fma, -ffp-contract=off):
//     div   = G^T y
//     !WEIGHTED:  t = div - f;           r = 1/(1 + tau_k) (tabulated)
//      WEIGHTED:  t = fma(-w, f, div);   r = 1.0 / fma(tau_k, w, 1.0) (IEEE division); step table with gamma = min w
//     x_new = fma(-tau_k, t, x) * r;     xbar = fma(-omega_k, x, (1 + omega_k)*x_new)
//     z     = fma(sigma_k, G xbar, y)
//     TAPE:       store z1, z2 (WEIGHTED: and x_new) of the core pixels: [k][component][image][pixel], private
//     n2    = fma(z2, z2, z1*z1);  out = n2 > alpha^2;   y = out ? z * (alpha*rsqrt_nr(n2)) : z
//      L1 (the data term w |u - f| in place of w/2 (u - f)^2; WEIGHTED's registers, tape and launch; step table with gamma = 0):
//                 v = fma(-tau_k, div, x);  d = v - f;  m = |d| - tau_k*w;  x_new = m > 0 ? f + copysign(m, d) : f
//      KL (the data term w (u - f log u), u >= 0, for Poisson noise; WEIGHTED's registers, tape and launch; gamma = 0):
//                 v = fma(-tau_k, div, x);  t = tau_k*w;  c = v - t;  g = t*f;  s = sqrt(c*c + 4*g)      (IEEE sqrt, division)
//                 x_new = c >= 0 ? 0.5*(c + s) : (2*g) / (s - c)
//                 (both are the positive root of u^2 - c u - t f = 0; the second has no cancellation when t is large.  c < 0
//                 gives s - c > 0: no guard.  w = 0 or f = 0: x_new = max(c, 0).  Out-of-image lanes: c = s = 0, x_new = 0)
// The two primal steps are two forms, not one with w = 1: each is pinned bit for bit.  !WEIGHTED gives bpltv_denoise's u
// (tests/test_gpu_unrolled.py), WEIGHTED bpltv_weighted_denoise's (tests/test_gpu_weighted_unrolled.py), whatever TAPE and
// TANGENT; and with w == 1.0 each weighted operation returns the bits of the one it replaces (tests/test_gpu_weighted.py).
//
// TANGENT, per pixel, beside iteration k, from dx = df, dy = 0 (no fma in it; the step table is held fixed):
//     ddiv = G^T dy
//     !WEIGHTED:  dt = ddiv - df
//      WEIGHTED:  dt = (ddiv - w*df) - dw*(f - x_new)
//     dxn  = (dx - tau_k*dt)*r;   dxb = (1 + omega_k)*dxn - omega_k*dx;   dx = dxn          (the primal's own r)
//      L1:        dv = dx - tau_k*ddiv;  act = x_new != f || w == 0;  dxn = act ? dv - tau_k*(sign(x_new - f)*dw) : df
//                 (the reverse tail's act and three-way sign, on x_new, f and w: a held pixel passes df and nothing else, a
//                 pixel without data passes dv)
//      KL:        dv = dx - tau_k*ddiv;  t = tau_k*w;  D = fma(t, f, x_new*x_new);  q = D > 0 ? x_new / D : 0;
//                 dxn = q*(x_new*dv + t*df + tau_k*((f - x_new)*dw))       (the reverse tail's D and q: x_new = 0 passes nothing)
//                 (both: dxb and dx as above; neither reads r)
//     dz   = dy + sigma_k * G dxb
//     out:  q = rsqrt_nr(n2); e = z*q; dot = e1*dz1 + e2*dz2; dy = dalpha*e + (alpha*q)*(dz - e*dot)   (the primal's decision)
//     else: dy = dz
// and du = dx after the last step (rsqrt_nr is differentiated as 1/sqrt(n2), here and in the reverse sweep).
//
// Reverse, per pixel, k = K-1 ... 0, from gx = dL/du, gy = gf = ga = gw = 0 (fma only where written):
//     n2  = fma(z2, z2, z1*z1);  out = n2 > alpha^2                   (the forward's expression: the same decision)
//     out:  q = rsqrt_nr(n2); e = z*q; dot = e1*gy1 + e2*gy2; gz = (alpha*q)*(gy - e*dot); ga += dot
//     else: gz = gy
//     gxb = sigma_k * G^T gz;  gxn = gx + (1 + omega_k)*gxb
//     !WEIGHTED:  c = 1/(1 + tau_k) (tabulated);  gf += tau_k*c*gxn;  gy = gz - tau_k*c * G gxn;  gx = c*gxn - omega_k*gxb
//      WEIGHTED:  r = 1.0 / fma(tau_k, w, 1.0);  h = gxn*r;  gf += tau_k*(w*h);  gw += tau_k*((f - x_{k+1})*h);
//                 gy = gz - tau_k * G h;  gx = h - omega_k*gxb
//      L1:        act = x_{k+1} != f || w == 0;  h = act ? gxn : 0;  gf += act ? 0 : gxn;  gw += -tau_k*(sign(x_{k+1} - f)*h);
//                 gy = gz - tau_k * G h;  gx = h - omega_k*gxb                        (decided on the tape alone)
//                 (w == 0: the threshold is the identity, x_new = v whatever d is, and so is its derivative -- without it a
//                 pixel without data whose d is zero up to rounding would be read as held at f or not by that rounding)
//      KL:        t = tau_k*w;  D = fma(t, f, x_{k+1}*x_{k+1});  q = D > 0 ? x_{k+1} / D : 0;  e = q*gxn;  h = x_{k+1}*e;
//                 gf += t*e;  gw += tau_k*((f - x_{k+1})*e);  gy = gz - tau_k * G h;  gx = h - omega_k*gxb
//                 (e = gxn / s, since s = x+ + t f / x+: dx+/dv = x+/s, dx+/df = t/s, dx+/dw = tau (f - x+)/s, from the tape, f
//                 and w alone.  Exact wherever x+ > 0.  Convention: where x+ = 0 exactly -- possible only where w f = 0 and the
//                 iterate was clamped -- the tail passes nothing (q = 0); the one-sided terms tau w/|c| and tau f/|c| of grad_f
//                 and grad_w there, which the tape cannot give, are dropped)
// and dL/df = gf + gx after the last step (x_0 = f, y_0 = 0).  The two tails agree to rounding only at w = 1
// (tests/test_gpu_weighted_unrolled.py).  The weighted sweep needs no w > 0: a mask (w in {0, 1}) gets gradients in f, alpha, w.
//
// What the lines above leave open, as the kernels and oracle/taped_oracle.c have it (tests/test_gpu_taped_bits.py holds forward and
// tape to that oracle bit for bit and both sweeps to it within the families' bounds, on data that sit on every decision below):
//     G^T y  = (y1[i-1,j] - y1[i,j]) + (y2[i,j-1] - y2[i,j]), a neighbour outside the image is 0; y1 of the last image row and
//              y2 of the last column are 0 because G's rows there are (forward: they never leave 0; reverse: gz enters as 0)
//     G x    = (x[i+1,j] - x[i,j], x[i,j+1] - x[i,j]), 0 at i = M-1 / j = N-1 (pdhg_x_pass / pdhg_y_pass of oracle/bpltv_oracle.c)
//     1 + omega_k is the table's fifth entry wherever it appears (xbar, dxb, gxn); tau_k*c is one product, formed first
//     sign(x_new - f) is three-way, +1 / -1 / 0, in the tangent and in the reverse tail; sign 0 adds -tau*0 to gw: nothing
//     the tape holds z before the projection (and x_new); ga += dot only where out
// Ties.  out = n2 > alpha^2 is strict: a dual exactly on the ball is not projected and passes its tangent and cotangent whole,
// in all three kernels (8-bit data reach n2 == alpha^2 only by construction, n2 == 0 on every flat patch: rsqrt_nr(0) must reach
// no result, also in a wave whose other lanes project).  L1: m == 0 holds the pixel at f; act is read off x_new, f and w and not
// off m, so a step let through that rounds back to f counts as held (forward and sweeps agree: both read x_new); w == 0 with
// d == 0 -- every pixel without data in iteration 0, and on flat patches later -- is act with sign 0.  KL: x_new == 0 exactly
// needs w f == 0 and c <= 0, then D == 0 and q = 0: tangent and reverse pass nothing through the data step, gw gets exactly 0 from
// it and du of a pixel clamped in the last iteration is exactly 0; 0/0 is never formed.
#pragma once
#include <hip/hip_runtime.h>

#include "pdhg_kernels.hpp"

namespace bpltv {

constexpr int TV_R = 32;        // region (core + halo) of one workgroup: 32 x 32 pixels, one per thread
constexpr int TV_REV_T = 8;     // most reverse iterations per launch: their taped values sit in registers (2 or 3 x 8 doubles)
constexpr size_t tv_lds_bytes() { return pdhg_lds_bytes(TV_R, TV_R); }   // one set of dynamic planes; the step rows are static
constexpr size_t tv_tangent_lds_bytes() { return 2 * tv_lds_bytes(); }   // TANGENT: primal planes, then the tangent's

struct TvTileArgs {
    const double* in[6];    // x, y1, y2 (TANGENT: and dx, dy1, dy2) of the state set read (not read by a first launch)
    double* out[6];
    const double* f;        // the dataset, O planes
    const double* w;        // WEIGHTED: fidelity weight, one plane (wstride 0) or O planes (wstride M*N)
    const double* alpha;    // am*an doubles, column major
    const double* tab;      // [maxiter][TAB_STRIDE] (WEIGHTED: the row's 1/(1 + tau) is not read)
    double* tape;           // TAPE: [maxiter][2 or 3][O][M*N]
    const double* df;       // TANGENT: O planes, or nullptr: a zero tangent
    const double* dw;       // TANGENT and WEIGHTED: planes as w, or nullptr
    const double* dalpha;   // TANGENT: am*an doubles, indexed as alpha, or nullptr
    size_t plane;           // O * M*N: doubles of one tape component
    size_t wstride;
    int am, an;
    int istride;            // !WEIGHTED: doubles between per-image blocks of alpha and of dalpha: 0 = one block for every image,
                            // am*an = image k reads block k
    int it0, nit;
    int tk0;                // tape base iteration: iteration k lives in slot k - tk0 (0: the full tape; a checkpointed sweep's
                            // segment tape starts at its segment's first iteration).  tab stays indexed by k itself
    int M, N;
    int halo;
    int first;              // 1: start from x = f, dx = df, y = dy = 0
    int img0;               // first image of this launch (grid.z = images of the launch chain)
};

// One workgroup per tile, grid (nTi, nTj, images), block 1024.  pdhg_tile_kernel<double, 1, 1, 32, 32>'s structure: state,
// f, w and alpha in registers for the whole launch, neighbour values through three LDS planes (y1 with a zero guard
// column, y2 with a zero guard row, xbar with pad cells), two barriers per iteration, the launch's step rows in LDS, the
// core written back, halo waves that are past their use keep the barriers company only.
// TAPE: two or three stores per iteration for the core pixels (valid in every iteration of a launch).
// TANGENT: a second set of LDS planes (same layout, same zero guards) for the tangent duals and dxb, written in front of the
// same two barriers as the primal ones.  Out-of-image lanes hold zero in every value (w = 0 there: r = 1) and keep it.
template <bool WEIGHTED, bool TAPE, bool TANGENT, bool L1 = false, bool KL = false>
__global__ __launch_bounds__(TV_R * TV_R) void tv_tile_kernel(TvTileArgs A) {
    static_assert(!(TAPE && TANGENT), "the tangent sweep records nothing");
    static_assert(!L1 || WEIGHTED, "the L1 data term takes the weighted model's w and tape");
    static_assert(!KL || (WEIGHTED && !L1), "the KL data term takes the weighted model's w and tape, and is not L1");
    constexpr int RI = TV_R, RJ = TV_R, S1 = RI + 1;
    constexpr int PLANES = RJ * S1 + (RJ + 1) * RI + RJ * RI + RI + 1;   // doubles of one set of planes (pdhg_lds_bytes)
    static_assert(PLANES * sizeof(double) == tv_lds_bytes(), "the plane layout is pdhg_lds_bytes'");
    constexpr int NC = WEIGHTED ? 3 : 2;             // tape components
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];
    double* smem = reinterpret_cast<double*>(tv_smem);
    double* sy1 = smem;                              // [RJ][S1]
    double* sy2 = smem + RJ * S1;                    // [RJ+1][RI]
    double* sxb = smem + RJ * S1 + (RJ + 1) * RI;    // [RJ][RI] + RI + 1
    double* sd1 = sy1 + PLANES;                      // TANGENT: the tangent's planes
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
    // address and are zeroed afterwards (they stay 0).
    const int gi = min(oi + li, M - 1), gj = min(oj + lj, N - 1);
    const size_t pix = gi + (size_t)M * gj;
    // image img's block (the global image index: a launch chain starts at img0); the weighted model has no per-image form
    size_t ai = WEIGHTED ? 0 : (size_t)img * (size_t)A.istride;
    if (amode == 2) {
        ai += pix;
    } else if (amode == 1) {
        const unsigned pa = ((unsigned)gi * (unsigned)A.am) / (unsigned)M;
        const unsigned pb = ((unsigned)gj * (unsigned)A.an) / (unsigned)N;
        ai += pa + (size_t)A.am * pb;
    }
    double x = 0.0, y1 = 0.0, y2 = 0.0, dx = 0.0, dy1 = 0.0, dy2 = 0.0;
    if (!first) {
        x = A.in[0][base + pix];
        y1 = A.in[1][base + pix];
        y2 = A.in[2][base + pix];
        if constexpr (TANGENT) {
            dx = A.in[3][base + pix];
            dy1 = A.in[4][base + pix];
            dy2 = A.in[5][base + pix];
        }
    }
    double f = A.f[base + pix];
    double w = 0.0, df = 0.0, dw = 0.0, dal = 0.0;
    if constexpr (WEIGHTED) w = A.w[(size_t)img * A.wstride + pix];
    if constexpr (TANGENT) {
        if (A.df) df = A.df[base + pix];
        if constexpr (WEIGHTED)
            if (A.dw) dw = A.dw[(size_t)img * A.wstride + pix];
    }
    double al = A.alpha[ai];
    if constexpr (TANGENT)
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
    if constexpr (TANGENT) {
        sd1[lj * S1 + li + 1] = dy1;
        sd2[(lj + 1) * RI + li] = dy2;
    }
    if (tid < RJ) {
        sy1[tid * S1] = 0.0;
        if constexpr (TANGENT) sd1[tid * S1] = 0.0;
    }
    if (tid < RI) {
        sy2[tid] = 0.0;
        if constexpr (TANGENT) sd2[tid] = 0.0;
    }
    if (tid < RI + 1) {
        sxb[RI * RJ + tid] = 0.0;
        if constexpr (TANGENT) sdb[RI * RJ + tid] = 0.0;
    }
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
    double* tz = TAPE ? A.tape + (size_t)NC * A.plane * (A.it0 - A.tk0) + idx : nullptr;
    // halo rows do not need all the iterations (pdhg_tile_kernel): a wave owns two adjacent rows; core rows run them all.
    // Every wave executes two barriers for each of the launch's nit iterations: loop_nit in the first loop, the rest in the
    // second.
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    const double wdf = w * df;   // TANGENT and WEIGHTED (the same product in every iteration)
    // r: the tabulated 1/(1 + tau) of the row, or (WEIGHTED) computed per pixel in the iteration
    double tau = srow[0], sigma = srow[1], omega = srow[2], r = srow[3], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step: x <- prox_{tau * fidelity}(x - tau * G^T y); over-relaxation (and their tangent)
        const double y1m = sy1[lj * S1 + li];
        const double y2m = sy2[lj * RI + li];
        double dy1m = 0.0, dy2m = 0.0;
        if constexpr (TANGENT) {
            dy1m = sd1[lj * S1 + li];
            dy2m = sd2[lj * RI + li];
        }
        const double div = (y1m - y1) + (y2m - y2);
        const double xo = x;
        double xn;
        if constexpr (L1) {   // soft threshold around f: no division, no r
            const double v = __builtin_fma(-tau, div, xo);
            const double d = v - f;
            const double m = __builtin_fabs(d) - tau * w;
            xn = (m > 0.0) ? f + __builtin_copysign(m, d) : f;
        } else if constexpr (KL) {   // the positive root of u^2 - c u - tau w f = 0, in the form without cancellation; no r
            const double v = __builtin_fma(-tau, div, xo);
            const double t = tau * w;
            const double c = v - t;
            const double g = t * f;
            const double s = __builtin_sqrt(c * c + 4.0 * g);
            xn = (c >= 0.0) ? 0.5 * (c + s) : (2.0 * g) / (s - c);
        } else {
            double t;
            if constexpr (WEIGHTED) {
                t = __builtin_fma(-w, f, div);
                r = 1.0 / __builtin_fma(tau, w, 1.0);
            } else {
                t = div - f;
            }
            xn = __builtin_fma(-tau, t, xo) * r;
        }
        const double b = __builtin_fma(-omega, xo, opw * xn);
        x = xn;
        double db = 0.0;
        if constexpr (TANGENT) {
            const double ddiv = (dy1m - dy1) + (dy2m - dy2);
            double dxn;
            if constexpr (L1) {   // the threshold's derivative, decided on x+, f and w as the reverse tail decides it from the tape
                const double dv = dx - tau * ddiv;
                const bool act = xn != f || w == 0.0;   // let through, or no threshold at all (w == 0: the identity)
                const double sdw = (xn > f) ? dw : ((xn < f) ? -dw : 0.0);
                dxn = act ? dv - tau * sdw : df;        // a held pixel moves with f and with nothing else
            } else if constexpr (KL) {   // dx+/dv = x+/s, dx+/df = t/s, dx+/dw = tau (f - x+)/s with 1/s = x+/D: the reverse tail's q
                const double dv = dx - tau * ddiv;
                const double t = tau * w;
                const double D = __builtin_fma(t, f, xn * xn);
                const double q = (D > 0.0) ? xn / D : 0.0;   // x+ = 0: the step passes nothing (the convention)
                dxn = q * (xn * dv + t * df + tau * ((f - xn) * dw));
            } else {
                double dt;
                if constexpr (WEIGHTED) dt = (ddiv - wdf) - dw * (f - xn);
                else dt = ddiv - df;
                dxn = (dx - tau * dt) * r;
            }
            db = opw * dxn - omega * dx;
            dx = dxn;
        }
        sxb[l] = b;
        if constexpr (TANGENT) sdb[l] = db;
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], nopw = nrow[4];
        if constexpr (!WEIGHTED) r = nrow[3];
        // ---- dual step: y <- proj_{|y_ij| <= alpha_ij}(y + sigma * G xbar) (and the projection's derivative)
        const double d1 = sxb[n1] - b;
        const double d2 = sxb[n2] - b;
        double y1n = __builtin_fma(sigma, d1, y1);
        double y2n = __builtin_fma(sigma, d2, y2);
        double dz1 = 0.0, dz2 = 0.0;
        if constexpr (TANGENT) {
            const double dd1 = sdb[n1] - db;
            const double dd2 = sdb[n2] - db;
            dz1 = dy1 + sigma * dd1;
            dz2 = dy2 + sigma * dd2;
        }
        if constexpr (TAPE) {
            if (core) {   // the tape: the dual before the projection (WEIGHTED: and the primal iterate grad_w reads)
                __hip_atomic_store(tz, y1n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(tz + A.plane, y2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (WEIGHTED) __hip_atomic_store(tz + 2 * A.plane, xn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            tz += NC * A.plane;
        }
        const double nn = __builtin_fma(y2n, y2n, y1n * y1n);
        const bool outp = nn > al * al;
        if (outp) {   // a wave whose pixels all lie inside the ball skips the rsqrt
            const double q = rsqrt_nr(nn);
            const double v = al * q;
            if constexpr (TANGENT) {
                const double e1 = y1n * q, e2 = y2n * q;
                const double dot = e1 * dz1 + e2 * dz2;
                dz1 = dal * e1 + v * (dz1 - e1 * dot);
                dz2 = dal * e2 + v * (dz2 - e2 * dot);
            }
            y1n = y1n * v;
            y2n = y2n * v;
        }
        y1 = y1n;
        y2 = y2n;
        sy1[lj * S1 + li + 1] = y1;
        sy2[(lj + 1) * RI + li] = y2;
        if constexpr (TANGENT) {
            dy1 = dz1;
            dy2 = dz2;
            sd1[lj * S1 + li + 1] = dy1;
            sd2[(lj + 1) * RI + li] = dy2;
        }
        tau = ntau; sigma = nsigma; omega = nomega; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    if (core) {
        // write-through stores, as pdhg_tile_kernel: the next launch reads this state from other XCDs
        __hip_atomic_store(&A.out[0][idx], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[1][idx], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[2][idx], y2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (TANGENT) {
            __hip_atomic_store(&A.out[3][idx], dx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[4][idx], dy1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[5][idx], dy2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct TvTileRevArgs {
    const double* in[3];    // gx, gy1, gy2 of the state set read; a first launch reads in[0] only: the cotangent dL/du
    double* out[3];
    double* gf;             // in place, owning core only
    double* ga;             // in place, owning core only: per-pixel parameter gradient
    double* gw;             // WEIGHTED: in place, owning core only: per-pixel, per-image weight gradient; nullptr: not wanted
    const double* tape;     // [maxiter][2 or 3][O][M*N]
    const double* f;        // WEIGHTED: the dataset; read only when gw is wanted (L1, KL: always)
    const double* w;        // WEIGHTED
    const double* alpha;
    const double* tab;
    size_t plane;
    size_t wstride;
    int am, an;
    int istride;            // as TvTileArgs
    int khi, nit;           // this launch runs the iterations khi, khi - 1, ..., khi - nit + 1
    int tk0;                // tape base iteration, as TvTileArgs (the launch stays inside the tape: khi - nit + 1 >= tk0)
    int M, N;
    int halo;
    int first;              // 1: start from gx = in[0], gy = gf = ga = gw = 0
    int img0;
};

// The mirror image: same region, halo and tile_span, nit <= TV_REV_T reverse iterations per launch, each reaching one pixel
// in each axis.  gx, gy1, gy2 ping-pong between two state sets (neighbouring tiles read each other's halos); gf, ga and gw are
// read and written by the owning core only.  gz1 goes through a plane with a zero guard column and gz2 through one with a zero
// guard row (G^T: neighbours i-1, j-1); gxn (WEIGHTED: h = r o gxn) through the padded plane (G: neighbours i+1, j+1) -- the
// layouts of sy1, sy2, sxb.  Out-of-image lanes stay zero (w = 0 there: r = 1): the duals of the last image row / column
// enter the planes as 0, as G^T treats them.  w and f are loaded once per launch.
template <bool WEIGHTED, bool L1 = false, bool KL = false>
__global__ __launch_bounds__(TV_R * TV_R) void tv_reverse_tile_kernel(TvTileRevArgs A) {
    static_assert(!L1 || WEIGHTED, "the L1 data term takes the weighted model's w and tape");
    static_assert(!KL || (WEIGHTED && !L1), "the KL data term takes the weighted model's w and tape, and is not L1");
    constexpr int RI = TV_R, RJ = TV_R, S1 = RI + 1;
    constexpr int NC = WEIGHTED ? 3 : 2;             // tape components
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];
    double* smem = reinterpret_cast<double*>(tv_smem);
    double* sg1 = smem;                              // [RJ][S1]
    double* sg2 = smem + RJ * S1;                    // [RJ+1][RI]
    double* sxn = smem + RJ * S1 + (RJ + 1) * RI;    // [RJ][RI] + RI + 1
    __shared__ __attribute__((aligned(16))) double srow[TV_REV_T * TAB_STRIDE];

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
    const bool want_w = WEIGHTED && A.gw != nullptr;   // (uniform)
    const bool want_x = L1 || KL || want_w;            // L1: the taped iterate and f decide the branch, whatever is wanted;
                                                       // KL: they are the derivative's denominator
    const int nit = A.nit;
    const int klo = A.khi - nit + 1;

    // ---- prologue: every global load, the launch's taped values included, is issued before the first use
    const int gi = min(oi + li, M - 1), gj = min(oj + lj, N - 1);
    const size_t pix = gi + (size_t)M * gj;
    size_t ai = WEIGHTED ? 0 : (size_t)img * (size_t)A.istride;   // as tv_tile_kernel
    if (amode == 2) {
        ai += pix;
    } else if (amode == 1) {
        const unsigned pa = ((unsigned)gi * (unsigned)A.am) / (unsigned)M;
        const unsigned pb = ((unsigned)gj * (unsigned)A.an) / (unsigned)N;
        ai += pa + (size_t)A.am * pb;
    }
    const int qi = oi + li, qj = oj + lj;
    const bool in = (qi < M) && (qj < N);
    const bool core = qi >= ci0 && qi < ci1 && qj >= cj0 && qj < cj1;
    double gx = A.in[0][base + pix], gy1 = 0.0, gy2 = 0.0, gf = 0.0, ga = 0.0, gw = 0.0;
    if (!first) {
        gy1 = A.in[1][base + pix];
        gy2 = A.in[2][base + pix];
        if (core) {
            gf = A.gf[base + pix];
            ga = A.ga[base + pix];
            if (want_w) gw = A.gw[base + pix];
        }
    }
    double al = A.alpha[ai];
    double w = 0.0, f = 0.0;
    if constexpr (WEIGHTED) w = A.w[(size_t)img * A.wstride + pix];
    if (want_x) f = A.f[base + pix];
    double z1[TV_REV_T], z2[TV_REV_T], xp[TV_REV_T];   // [s]: iteration khi - s (xp: the primal iterate, for gw)
    const double* tz = A.tape + (size_t)NC * A.plane * (A.khi - A.tk0) + base + pix;
#pragma unroll
    for (int s = 0; s < TV_REV_T; ++s) {
        z1[s] = 0.0; z2[s] = 0.0; xp[s] = 0.0;
        if (s < nit) {
            z1[s] = tz[0];
            z2[s] = tz[A.plane];
            if (want_x) xp[s] = tz[2 * A.plane];
        }
        tz -= NC * A.plane;
    }
    const bool row_word = tid < nit * TAB_STRIDE;   // nit <= TV_REV_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * klo + tid];
    if (!in) { gx = 0.0; gy1 = 0.0; gy2 = 0.0; al = 0.0; w = 0.0; }
    if (tid < RJ) sg1[tid * S1] = 0.0;
    if (tid < RI) sg2[tid] = 0.0;
    if (tid < RI + 1) sxn[RI * RJ + tid] = 0.0;
    if (row_word) srow[tid] = row_w;
    __syncthreads();

    const int l = lj * RI + li;
    const bool e1 = qi < M - 1, e2 = qj < N - 1;   // the pixel has a forward difference along i / j
    const int n1 = l + (e1 ? 1 : 0);
    const int n2 = l + (e2 ? RI : 0);
    const double a2 = al * al;
#pragma unroll
    for (int s = 0; s < TV_REV_T; ++s) {
        if (s < nit) {   // (uniform)
            const double* row = srow + TAB_STRIDE * (nit - 1 - s);
            const double tau = row[0], sigma = row[1], omega = row[2], c = row[3], opw = row[4];   // (c: !WEIGHTED only)
            // ---- adjoint of the projection, on the taped dual
            const double za = in ? z1[s] : 0.0, zb = in ? z2[s] : 0.0;
            const double nn = __builtin_fma(zb, zb, za * za);
            double gz1 = gy1, gz2 = gy2;
            if (nn > a2) {
                const double q = rsqrt_nr(nn);
                const double u1 = za * q, u2 = zb * q;
                const double dot = u1 * gy1 + u2 * gy2;
                const double v = al * q;
                gz1 = v * (gy1 - u1 * dot);
                gz2 = v * (gy2 - u2 * dot);
                ga += dot;
            }
            const double m1 = e1 ? gz1 : 0.0, m2 = e2 ? gz2 : 0.0;
            sg1[lj * S1 + li + 1] = m1;
            sg2[(lj + 1) * RI + li] = m2;
            __syncthreads();
            // ---- adjoint of the over-relaxation and the primal step
            const double gt = (sg1[lj * S1 + li] - m1) + (sg2[lj * RI + li] - m2);
            const double gxb = sigma * gt;
            const double gxn = gx + opw * gxb;
            if constexpr (L1) {
                const double xk = xp[s];
                const bool act = in && (xk != f || w == 0.0);   // the threshold let the step through, or there is none (w == 0:
                                                                // the identity); out-of-image lanes stay zero
                const double h = act ? gxn : 0.0;
                sxn[l] = h;
                __syncthreads();
                const double d1 = sxn[n1] - h;
                const double d2 = sxn[n2] - h;
                gf += act ? 0.0 : gxn;
                if (want_w) gw += -tau * ((xk > f) ? h : ((xk < f) ? -h : 0.0));   // (x+ == f with w == 0: d = 0, no side)
                gy1 = gz1 - tau * d1;
                gy2 = gz2 - tau * d2;
                gx = h - omega * gxb;
            } else if constexpr (KL) {
                const double xk = in ? xp[s] : 0.0;   // out-of-image lanes stay zero (f is the clamped pixel's there; D > 0 then)
                const double t = tau * w;
                const double D = __builtin_fma(t, f, xk * xk);
                const double q = (D > 0.0) ? xk / D : 0.0;   // x+ = 0: the tail passes nothing (the convention)
                const double e = q * gxn;
                const double h = xk * e;
                sxn[l] = h;
                __syncthreads();
                const double d1 = sxn[n1] - h;
                const double d2 = sxn[n2] - h;
                gf += t * e;
                if (want_w) gw += tau * ((f - xk) * e);
                gy1 = gz1 - tau * d1;
                gy2 = gz2 - tau * d2;
                gx = h - omega * gxb;
            } else if constexpr (WEIGHTED) {
                const double r = 1.0 / __builtin_fma(tau, w, 1.0);
                const double h = gxn * r;
                sxn[l] = h;
                __syncthreads();
                const double d1 = sxn[n1] - h;
                const double d2 = sxn[n2] - h;
                gf += tau * (w * h);
                if (want_w) gw += tau * ((f - xp[s]) * h);
                gy1 = gz1 - tau * d1;
                gy2 = gz2 - tau * d2;
                gx = h - omega * gxb;
            } else {
                sxn[l] = gxn;
                __syncthreads();
                const double d1 = sxn[n1] - gxn;
                const double d2 = sxn[n2] - gxn;
                const double tc = tau * c;
                gf += tc * gxn;
                gy1 = gz1 - tc * d1;
                gy2 = gz2 - tc * d2;
                gx = c * gxn - omega * gxb;
            }
        }
    }

    if (core) {
        const size_t idx = base + qi + (size_t)M * qj;
        __hip_atomic_store(&A.out[0][idx], gx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[1][idx], gy1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.out[2][idx], gy2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.gf[idx], gf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.ga[idx], ga, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (want_w) __hip_atomic_store(&A.gw[idx], gw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// dL/df = gf + gx after the last reverse step (x_0 = f)
__global__ __launch_bounds__(256) void unrolled_gradf_kernel(const double* __restrict__ gf, const double* __restrict__ gx, size_t n,
                                                             double* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[q] = gf[q] + gx[q];
}

}  // namespace bpltv
