// color_tile_kernels.hpp -- channel-coupled (vectorial) TV on a 32 x 32 region: tv_tile_kernel<0, TAPE, 0> and
// tv_reverse_tile_kernel<0> (tv_tile_kernels.hpp) with the projection taken over the C consecutive planes of a colour image.
// The reference has no counterpart: its datasets are grey.  DESIGN.md section 4.12.
//
//     min_u  1/2 sum_c |u_c - f_c|^2  +  sum_pixels alpha * sqrt( sum_c |(grad u_c)|^2 )
//
// Layout: a handle of O = B*C planes; colour image b owns the planes b*C ... b*C + C-1.  alpha is shared by the batch and by
// the channels (scalar, patch or map).
//
// Forward, per plane c of a colour image, iteration k = 0 ... K-1 from x = f, y = 0: div, t, x_new, xbar and
// z = fma(sigma_k, G xbar, y) are tv_tile_kernel's !WEIGHTED forms, operation for operation.  Then, per pixel of the colour
// image, over its planes in channel order:
//     n2 = z1_0*z1_0;  n2 = fma(z2_0, z2_0, n2);   c = 1 ... C-1:  n2 = fma(z1_c, z1_c, n2);  n2 = fma(z2_c, z2_c, n2)
//     out = n2 > alpha^2;   y_c = out ? z_c * (alpha*rsqrt_nr(n2)) : z_c   for every c
// With C = 1 this is tv_tile_kernel's expression; channels = 1 runs the TV kernels themselves.
// TAPE: z1, z2 of every plane before the projection, in the TV tape's layout, [k][component][plane][pixel].
//
// Reverse, k = K-1 ... 0, from gx = dL/du, gy = gf = ga = 0: n2 and out as above on the taped values; where out:
//     q = rsqrt_nr(n2);  e_c = z_c*q;  dot = (e1_0*gy1_0 + e2_0*gy2_0), then dot += (e1_c*gy1_c + e2_c*gy2_c), c = 1 ... C-1
//     gz_c = (alpha*q)*(gy_c - e_c*dot);  ga += dot       (once per pixel of the colour image)
// elsewhere gz = gy.  The rest is tv_reverse_tile_kernel<0>'s tail, per plane.  ga is written into the colour image's
// channel-0 plane of the driver's ga planes and +0.0 into the others, so that the TV reduction sums colour images in image
// order.
//
// One workgroup per (tile, colour image): 1024 threads, one pixel per thread with its C channels in registers.  LDS: C sets
// of the TV planes.  Two barriers per iteration, every load first, the step rows in LDS, spent halo waves keep the barriers
// company only, agent-scope write-through stores of the core: tv_tile_kernel's structure.
// color_tangent_tile_kernel<C> (below) carries the tangent through the same iterations: DESIGN.md section 4.13.
//
// WEIGHTED: the fidelity 1/2 sum_c sum_pixels w_c (u_c - f_c)^2, w >= 0, one weight plane for all planes
// or one per plane.  The primal step of every plane is tv_tile_kernel<1, ...>'s -- t = fma(-w_c, f_c, div), r_c = 1.0 / fma(tau_k,
// w_c, 1.0), x_new = fma(-tau_k, t, x) * r_c -- the projection stays the one above, and the tape also holds x_new of every plane
// ([k][z1, z2, x][plane][pixel]).  Reverse: the projection adjoint above, then tv_reverse_tile_kernel<1>'s tail per plane:
//     h = gxn*r_c;  gf += tau_k*(w_c*h);  gw_c += tau_k*((f_c - x_new_c)*h);  gy = gz - tau_k * G h;  gx = h - omega_k*gxb
// With w == 1.0 every weighted operation returns the bits of the one it replaces.
#pragma once
#include <hip/hip_runtime.h>

#include "tv_tile_kernels.hpp"

namespace bpltv {

constexpr int COLOR_MAX_C = 4;
// Most reverse iterations per launch: 2*C*T taped doubles sit in registers beside 5*C doubles of sweep state, in the 128
// VGPRs a lane of a 1024-thread workgroup has.  The deepest that leaves no instantiation with scratch: 96 / 108 / 118 VGPRs
// (4 / 3 / 2 take 80 / 96 / 102 and a sweep 14 % longer).
constexpr int color_rev_t(int C) { return C <= 1 ? TV_REV_T : (C == 2 ? 6 : (C == 3 ? 4 : 3)); }
constexpr size_t color_lds_bytes(int C) { return (size_t)C * tv_lds_bytes(); }

// The weighted sweep also holds x+ of every taped iteration (for gw) beside w and f: 3*C*T taped doubles and 8*C of sweep state,
// weight and data.  The deepest that leaves no instantiation with scratch: 119 / 112 / 106 VGPRs (one
// more iteration spills 20 / 12 / 52 bytes per lane).
constexpr int color_weighted_rev_t(int C) { return C <= 1 ? TV_REV_T : (C == 2 ? 5 : (C == 3 ? 2 : 1)); }

// TvTileArgs with: img0 / grid.z count colour images; in, out, f, tape address the planes img*C + c; df, dw, dalpha and istride
// are not read.  WEIGHTED: w is one plane (wstride 0) or O planes (wstride M*N: plane img*C + c), the
// primal step of every plane is tv_tile_kernel<1, ...>'s and the tape has its three components; otherwise w and wstride are not
// read.
template <int C, bool TAPE, bool WEIGHTED = false>
__global__ __launch_bounds__(TV_R * TV_R) void color_tile_kernel(TvTileArgs A) {
    static_assert(C >= 2 && C <= COLOR_MAX_C, "channels = 1 is tv_tile_kernel");
    constexpr int RI = TV_R, RJ = TV_R, S1 = RI + 1;
    constexpr int PLANES = RJ * S1 + (RJ + 1) * RI + RJ * RI + RI + 1;   // doubles of one channel's planes (pdhg_lds_bytes)
    static_assert(PLANES * sizeof(double) == tv_lds_bytes(), "the plane layout is pdhg_lds_bytes'");
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];
    double* sy1 = reinterpret_cast<double*>(tv_smem);   // [RJ][S1]               channel c: + c * PLANES
    double* sy2 = sy1 + RJ * S1;                        // [RJ+1][RI]
    double* sxb = sy2 + (RJ + 1) * RI;                  // [RJ][RI] + RI + 1
    __shared__ __attribute__((aligned(16))) double srow[PDHG_MAX_T * TAB_STRIDE];

    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y, img = A.img0 + (int)blockIdx.z;
    const int M = A.M, N = A.N;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, N, RJ, A.halo, oj, cj0, cj1);
    const size_t npx = (size_t)M * N;
    const size_t base = (size_t)img * C * npx;   // channel 0 of the colour image
    const int amode = (A.am == 1 && A.an == 1) ? 0 : ((A.am == M && A.an == N) ? 2 : 1);
    const bool first = A.first != 0;

    // ---- prologue: every global load is issued before the first use.  Out-of-image pixels read a clamped in-image
    // address and are zeroed afterwards (they stay 0).
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
    double x[C], y1[C], y2[C], f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        x[c] = 0.0; y1[c] = 0.0; y2[c] = 0.0;
        if (!first) {
            x[c] = A.in[0][base + c * npx + pix];
            y1[c] = A.in[1][base + c * npx + pix];
            y2[c] = A.in[2][base + c * npx + pix];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = A.f[base + c * npx + pix];
    double w[WEIGHTED ? C : 1];   // WEIGHTED: the weight of every channel (one plane: the same value C times)
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int c = 0; c < C; ++c) w[c] = A.w[(size_t)(img * C + c) * A.wstride + pix];
    }
    double al = A.alpha[ai];
    const bool row_word = tid < A.nit * TAB_STRIDE;   // nit <= PDHG_MAX_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * A.it0 + tid];
    const bool in = (oi + li < M) && (oj + lj < N);
    if (!in) al = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (first) { x[c] = f[c]; y1[c] = 0.0; y2[c] = 0.0; }
        if (!in) { f[c] = 0.0; x[c] = 0.0; y1[c] = 0.0; y2[c] = 0.0; }
        if constexpr (WEIGHTED)
            if (!in) w[c] = 0.0;   // r = 1 there: the lane stays zero
        sy1[c * PLANES + lj * S1 + li + 1] = y1[c];
        sy2[c * PLANES + (lj + 1) * RI + li] = y2[c];
        if (tid < RJ) sy1[c * PLANES + tid * S1] = 0.0;
        if (tid < RI) sy2[c * PLANES + tid] = 0.0;
        if (tid < RI + 1) sxb[c * PLANES + RI * RJ + tid] = 0.0;
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
    const size_t idx = base + qi + (size_t)M * qj;   // channel 0; used by core pixels only
    constexpr int NC = WEIGHTED ? 3 : 2;   // tape components
    double* tz = TAPE ? A.tape + (size_t)NC * A.plane * (A.it0 - A.tk0) + idx : nullptr;
    // halo rows do not need all the iterations (tv_tile_kernel): a wave owns two adjacent rows; core rows run them all
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    // r: the tabulated 1/(1 + tau) of the row, or (WEIGHTED) computed per plane in the iteration
    double tau = srow[0], sigma = srow[1], omega = srow[2], r = srow[3], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step of every channel
        double b[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double y1m = sy1[c * PLANES + lj * S1 + li];
            const double y2m = sy2[c * PLANES + lj * RI + li];
            const double div = (y1m - y1[c]) + (y2m - y2[c]);
            double t;
            if constexpr (WEIGHTED) {
                t = __builtin_fma(-w[c], f[c], div);
                r = 1.0 / __builtin_fma(tau, w[c], 1.0);
            } else {
                t = div - f[c];
            }
            const double xo = x[c];
            const double xn = __builtin_fma(-tau, t, xo) * r;
            b[c] = __builtin_fma(-omega, xo, opw * xn);
            x[c] = xn;
            sxb[c * PLANES + l] = b[c];
        }
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], nopw = nrow[4];
        if constexpr (!WEIGHTED) r = nrow[3];
        // ---- dual step: z of every channel, then one projection for the pixel
        double nn = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double d1 = sxb[c * PLANES + n1] - b[c];
            const double d2 = sxb[c * PLANES + n2] - b[c];
            y1[c] = __builtin_fma(sigma, d1, y1[c]);
            y2[c] = __builtin_fma(sigma, d2, y2[c]);
            if constexpr (TAPE) {
                if (core) {   // the tape: the dual before the projection (WEIGHTED: and the primal iterate grad_w reads)
                    __hip_atomic_store(tz + c * npx, y1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(tz + c * npx + A.plane, y2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if constexpr (WEIGHTED) __hip_atomic_store(tz + c * npx + 2 * A.plane, x[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            nn = (c == 0) ? y1[c] * y1[c] : __builtin_fma(y1[c], y1[c], nn);
            nn = __builtin_fma(y2[c], y2[c], nn);
        }
        if constexpr (TAPE) tz += NC * A.plane;
        if (nn > al * al) {   // a wave whose pixels all lie inside the ball skips the rsqrt
            const double v = al * rsqrt_nr(nn);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                y1[c] = y1[c] * v;
                y2[c] = y2[c] * v;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            sy1[c * PLANES + lj * S1 + li + 1] = y1[c];
            sy2[c * PLANES + (lj + 1) * RI + li] = y2[c];
        }
        tau = ntau; sigma = nsigma; omega = nomega; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    if (core) {
        // write-through stores, as tv_tile_kernel: the next launch reads this state from other XCDs
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __hip_atomic_store(&A.out[0][idx + c * npx], x[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[1][idx + c * npx], y1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[2][idx + c * npx], y2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The tangent sweep: color_tile_kernel<C, false> carrying tv_tile_kernel<0, 0, 1>'s tangent, with the
// derivative of the projection taken over the C planes of a colour image.  Per plane c, beside iteration k, from dx = df, dy = 0
// (no fma in it; the step table is held fixed):
//     ddiv_c = G^T dy_c;  dt_c = ddiv_c - df_c
//     dxn_c  = (dx_c - tau_k*dt_c)*r_k;   dxb_c = (1 + omega_k)*dxn_c - omega_k*dx_c;   dx_c = dxn_c
//     dz_c   = dy_c + sigma_k * G dxb_c
// then once per pixel of the colour image, on the primal's own n2 and decision:
//     out:  q = rsqrt_nr(n2);  e_c = z_c*q;  dot = (e1_0*dz1_0 + e2_0*dz2_0), then dot += (e1_c*dz1_c + e2_c*dz2_c), c = 1 ... C-1
//           dy_c = dalpha*e_c + (alpha*q)*(dz_c - e_c*dot)
//     else: dy_c = dz_c
// and du = dx after the last step: the transpose of color_reverse_tile_kernel's sweep.  The primal half is color_tile_kernel's,
// operation for operation.
//
// LDS: 2*C sets of planes, channel c's primal set at c, its tangent set at C + c.  Four channels of full TV sets (202 816 B)
// pass the 163 840 B of a CU, so a set keeps no y1 / dy1 plane: the left neighbour is lane li - 1 of the same 32-pixel row, and
// a wave holds two whole rows, so it comes by a lane shift (pd_lane_prev_or0) with the zero guard for li = 0.  That only moves
// data: the bits do not change.  Two and three channels would fit with the planes; the shift is not slower there (DESIGN.md
// section 4.13), so every instantiation has the one exchange.
constexpr size_t color_tangent_set_doubles() { return (TV_R + 1) * TV_R + TV_R * TV_R + TV_R + 1; }   // y2 and xbar planes
constexpr size_t color_tangent_lds_bytes(int C) { return (size_t)2 * C * color_tangent_set_doubles() * sizeof(double); }

// TvTileArgs as color_tile_kernel, with in / out of six planes (x, y1, y2, dx, dy1, dy2), df (the planes img*C + c) and dalpha
// (indexed as alpha); either may be nullptr: a zero tangent.  tape, w, dw, wstride and istride are not read.
template <int C>
__global__ __launch_bounds__(TV_R * TV_R) void color_tangent_tile_kernel(TvTileArgs A) {
    static_assert(C >= 2 && C <= COLOR_MAX_C, "channels = 1 is tv_tile_kernel<0, 0, 1>");
    constexpr int RI = TV_R, RJ = TV_R;
    constexpr int PLANES = (int)color_tangent_set_doubles();
    static_assert(color_tangent_lds_bytes(C) + PDHG_MAX_T * TAB_STRIDE * sizeof(double) <= 163840, "the LDS of a CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];
    double* sy2 = reinterpret_cast<double*>(tv_smem);   // [RJ+1][RI]             channel c: + c * PLANES
    double* sxb = sy2 + (RJ + 1) * RI;                  // [RJ][RI] + RI + 1
    double* sd2 = sy2 + C * PLANES;                     // the tangent's planes
    double* sdb = sxb + C * PLANES;
    __shared__ __attribute__((aligned(16))) double srow[PDHG_MAX_T * TAB_STRIDE];

    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y, img = A.img0 + (int)blockIdx.z;
    const int M = A.M, N = A.N;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, N, RJ, A.halo, oj, cj0, cj1);
    const size_t npx = (size_t)M * N;
    const size_t base = (size_t)img * C * npx;   // channel 0 of the colour image
    const int amode = (A.am == 1 && A.an == 1) ? 0 : ((A.am == M && A.an == N) ? 2 : 1);
    const bool first = A.first != 0;

    // ---- prologue: every global load is issued before the first use.  Out-of-image pixels read a clamped in-image
    // address and are zeroed afterwards (they stay 0).
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
    double x[C], y1[C], y2[C], f[C], dx[C], dy1[C], dy2[C], df[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        x[c] = 0.0; y1[c] = 0.0; y2[c] = 0.0; dx[c] = 0.0; dy1[c] = 0.0; dy2[c] = 0.0;
        if (!first) {
            x[c] = A.in[0][base + c * npx + pix];
            y1[c] = A.in[1][base + c * npx + pix];
            y2[c] = A.in[2][base + c * npx + pix];
            dx[c] = A.in[3][base + c * npx + pix];
            dy1[c] = A.in[4][base + c * npx + pix];
            dy2[c] = A.in[5][base + c * npx + pix];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        f[c] = A.f[base + c * npx + pix];
        df[c] = 0.0;
        if (A.df) df[c] = A.df[base + c * npx + pix];
    }
    double al = A.alpha[ai], dal = 0.0;
    if (A.dalpha) dal = A.dalpha[ai];
    const bool row_word = tid < A.nit * TAB_STRIDE;   // nit <= PDHG_MAX_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * A.it0 + tid];
    const bool in = (oi + li < M) && (oj + lj < N);
    if (!in) { al = 0.0; dal = 0.0; }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (first) { x[c] = f[c]; y1[c] = 0.0; y2[c] = 0.0; dx[c] = df[c]; dy1[c] = 0.0; dy2[c] = 0.0; }
        if (!in) { f[c] = 0.0; x[c] = 0.0; y1[c] = 0.0; y2[c] = 0.0; df[c] = 0.0; dx[c] = 0.0; dy1[c] = 0.0; dy2[c] = 0.0; }
        sy2[c * PLANES + (lj + 1) * RI + li] = y2[c];
        sd2[c * PLANES + (lj + 1) * RI + li] = dy2[c];
        if (tid < RI) { sy2[c * PLANES + tid] = 0.0; sd2[c * PLANES + tid] = 0.0; }
        if (tid < RI + 1) { sxb[c * PLANES + RI * RJ + tid] = 0.0; sdb[c * PLANES + RI * RJ + tid] = 0.0; }
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
    const size_t idx = base + qi + (size_t)M * qj;   // channel 0; used by core pixels only
    // halo rows do not need all the iterations (tv_tile_kernel): a wave owns two adjacent rows; core rows run them all
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    double tau = srow[0], sigma = srow[1], omega = srow[2], r = srow[3], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step of every channel, and its tangent
        double b[C], db[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            // lane li - 1 of the row (every lane of the wave is here); li = 0: the zero guard column
            const double p = pd_lane_prev_or0(y1[c]), dp = pd_lane_prev_or0(dy1[c]);
            const double y1m = li ? p : 0.0, dy1m = li ? dp : 0.0;
            const double y2m = sy2[c * PLANES + lj * RI + li];
            const double dy2m = sd2[c * PLANES + lj * RI + li];
            const double div = (y1m - y1[c]) + (y2m - y2[c]);
            const double t = div - f[c];
            const double xo = x[c];
            const double xn = __builtin_fma(-tau, t, xo) * r;
            b[c] = __builtin_fma(-omega, xo, opw * xn);
            x[c] = xn;
            const double ddiv = (dy1m - dy1[c]) + (dy2m - dy2[c]);
            const double dt = ddiv - df[c];
            const double dxn = (dx[c] - tau * dt) * r;
            db[c] = opw * dxn - omega * dx[c];
            dx[c] = dxn;
            sxb[c * PLANES + l] = b[c];
            sdb[c * PLANES + l] = db[c];
        }
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], nopw = nrow[4];
        r = nrow[3];
        // ---- dual step: z and dz of every channel (y becomes z, dy becomes dz), then one projection for the pixel
        double nn = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double d1 = sxb[c * PLANES + n1] - b[c];
            const double d2 = sxb[c * PLANES + n2] - b[c];
            y1[c] = __builtin_fma(sigma, d1, y1[c]);
            y2[c] = __builtin_fma(sigma, d2, y2[c]);
            const double dd1 = sdb[c * PLANES + n1] - db[c];
            const double dd2 = sdb[c * PLANES + n2] - db[c];
            dy1[c] = dy1[c] + sigma * dd1;
            dy2[c] = dy2[c] + sigma * dd2;
            nn = (c == 0) ? y1[c] * y1[c] : __builtin_fma(y1[c], y1[c], nn);
            nn = __builtin_fma(y2[c], y2[c], nn);
        }
        if (nn > al * al) {   // a wave whose pixels all lie inside the ball skips the rsqrt
            const double q = rsqrt_nr(nn);
            const double v = al * q;
            double e1[C], e2[C], dot = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                e1[c] = y1[c] * q;
                e2[c] = y2[c] * q;
                const double d = e1[c] * dy1[c] + e2[c] * dy2[c];
                dot = (c == 0) ? d : dot + d;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                dy1[c] = dal * e1[c] + v * (dy1[c] - e1[c] * dot);
                dy2[c] = dal * e2[c] + v * (dy2[c] - e2[c] * dot);
                y1[c] = y1[c] * v;
                y2[c] = y2[c] * v;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            sy2[c * PLANES + (lj + 1) * RI + li] = y2[c];
            sd2[c * PLANES + (lj + 1) * RI + li] = dy2[c];
        }
        tau = ntau; sigma = nsigma; omega = nomega; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    if (core) {
        // write-through stores, as tv_tile_kernel: the next launch reads this state from other XCDs
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __hip_atomic_store(&A.out[0][idx + c * npx], x[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[1][idx + c * npx], y1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[2][idx + c * npx], y2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[3][idx + c * npx], dx[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[4][idx + c * npx], dy1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[5][idx + c * npx], dy2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// TvTileRevArgs with: img0 / grid.z count colour images; in, out, gf, tape address the planes img*C + c; ga: the colour
// image's value in its channel-0 plane, +0.0 in the others; istride is not read.  nit <= color_rev_t(C).
// WEIGHTED: tv_reverse_tile_kernel<1>'s tail per plane -- h = r_c o gxn goes through the padded plane,
// gw into a plane of its own (nullptr: not wanted, and neither f nor the taped x+ is loaded); w as color_tile_kernel's; the
// tape has three components; nit <= color_weighted_rev_t(C).  Otherwise gw, f, w and wstride are not read.
template <int C, bool WEIGHTED = false>
__global__ __launch_bounds__(TV_R * TV_R) void color_reverse_tile_kernel(TvTileRevArgs A) {
    static_assert(C >= 2 && C <= COLOR_MAX_C, "channels = 1 is tv_reverse_tile_kernel");
    constexpr int RI = TV_R, RJ = TV_R, S1 = RI + 1;
    constexpr int PLANES = RJ * S1 + (RJ + 1) * RI + RJ * RI + RI + 1;
    constexpr int T = WEIGHTED ? color_weighted_rev_t(C) : color_rev_t(C);
    constexpr int NC = WEIGHTED ? 3 : 2;   // tape components
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];
    double* sg1 = reinterpret_cast<double*>(tv_smem);   // [RJ][S1]               channel c: + c * PLANES
    double* sg2 = sg1 + RJ * S1;                        // [RJ+1][RI]
    double* sxn = sg2 + (RJ + 1) * RI;                  // [RJ][RI] + RI + 1
    __shared__ __attribute__((aligned(16))) double srow[T * TAB_STRIDE];

    const int tid = threadIdx.x;
    const int li = tid % RI, lj = tid / RI;
    const int ta = (int)blockIdx.x, tb = (int)blockIdx.y, img = A.img0 + (int)blockIdx.z;
    const int M = A.M, N = A.N;
    int oi, ci0, ci1, oj, cj0, cj1;
    tile_span(ta, M, RI, A.halo, oi, ci0, ci1);
    tile_span(tb, N, RJ, A.halo, oj, cj0, cj1);
    const size_t npx = (size_t)M * N;
    const size_t base = (size_t)img * C * npx;
    const int amode = (A.am == 1 && A.an == 1) ? 0 : ((A.am == M && A.an == N) ? 2 : 1);
    const bool first = A.first != 0;
    const bool want_w = WEIGHTED && A.gw != nullptr;   // (uniform)
    const int nit = A.nit;
    const int klo = A.khi - nit + 1;

    // ---- prologue: every global load, the launch's taped values included, is issued before the first use
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
    const int qi = oi + li, qj = oj + lj;
    const bool in = (qi < M) && (qj < N);
    const bool core = qi >= ci0 && qi < ci1 && qj >= cj0 && qj < cj1;
    double gx[C], gy1[C], gy2[C], gf[C], ga = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        gx[c] = A.in[0][base + c * npx + pix];
        gy1[c] = 0.0; gy2[c] = 0.0; gf[c] = 0.0;
        if (!first) {
            gy1[c] = A.in[1][base + c * npx + pix];
            gy2[c] = A.in[2][base + c * npx + pix];
            if (core) gf[c] = A.gf[base + c * npx + pix];
        }
    }
    if (!first && core) ga = A.ga[base + pix];
    double gw[WEIGHTED ? C : 1], w[WEIGHTED ? C : 1], f[WEIGHTED ? C : 1];
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            gw[c] = 0.0; f[c] = 0.0;
            w[c] = A.w[(size_t)(img * C + c) * A.wstride + pix];
            if (want_w) {
                f[c] = A.f[base + c * npx + pix];
                if (!first && core) gw[c] = A.gw[base + c * npx + pix];
            }
        }
    }
    double al = A.alpha[ai];
    double z1[C][T], z2[C][T];   // [c][s]: iteration khi - s
    double xp[WEIGHTED ? C : 1][T];   // WEIGHTED: the primal iterate, for gw
    const double* tz = A.tape + (size_t)NC * A.plane * (A.khi - A.tk0) + base + pix;
#pragma unroll
    for (int s = 0; s < T; ++s) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            z1[c][s] = 0.0; z2[c][s] = 0.0;
            if (s < nit) {
                z1[c][s] = tz[c * npx];
                z2[c][s] = tz[c * npx + A.plane];
            }
            if constexpr (WEIGHTED) {
                xp[c][s] = 0.0;
                if (s < nit && want_w) xp[c][s] = tz[c * npx + 2 * A.plane];
            }
        }
        tz -= NC * A.plane;
    }
    const bool row_word = tid < nit * TAB_STRIDE;   // nit <= T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * klo + tid];
    if (!in) al = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (!in) { gx[c] = 0.0; gy1[c] = 0.0; gy2[c] = 0.0; }
        if constexpr (WEIGHTED)
            if (!in) w[c] = 0.0;   // r = 1 there: the lane stays zero
        if (tid < RJ) sg1[c * PLANES + tid * S1] = 0.0;
        if (tid < RI) sg2[c * PLANES + tid] = 0.0;
        if (tid < RI + 1) sxn[c * PLANES + RI * RJ + tid] = 0.0;
    }
    if (row_word) srow[tid] = row_w;
    __syncthreads();

    const int l = lj * RI + li;
    const bool e1 = qi < M - 1, e2 = qj < N - 1;   // the pixel has a forward difference along i / j
    const int n1 = l + (e1 ? 1 : 0);
    const int n2 = l + (e2 ? RI : 0);
    const double a2 = al * al;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        if (s < nit) {   // (uniform)
            const double* row = srow + TAB_STRIDE * (nit - 1 - s);
            const double tau = row[0], sigma = row[1], omega = row[2], cr = row[3], opw = row[4];
            // ---- adjoint of the projection, on the taped duals of the pixel's channels (gy becomes gz)
            double za[C], zb[C], nn = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                za[c] = in ? z1[c][s] : 0.0;
                zb[c] = in ? z2[c][s] : 0.0;
                nn = (c == 0) ? za[c] * za[c] : __builtin_fma(za[c], za[c], nn);
                nn = __builtin_fma(zb[c], zb[c], nn);
            }
            if (nn > a2) {
                const double q = rsqrt_nr(nn);
                double dot = 0.0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    za[c] = za[c] * q;
                    zb[c] = zb[c] * q;
                    const double d = za[c] * gy1[c] + zb[c] * gy2[c];
                    dot = (c == 0) ? d : dot + d;
                }
                const double v = al * q;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    gy1[c] = v * (gy1[c] - za[c] * dot);
                    gy2[c] = v * (gy2[c] - zb[c] * dot);
                }
                ga += dot;
            }
            double m1[C], m2[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                m1[c] = e1 ? gy1[c] : 0.0;
                m2[c] = e2 ? gy2[c] : 0.0;
                sg1[c * PLANES + lj * S1 + li + 1] = m1[c];
                sg2[c * PLANES + (lj + 1) * RI + li] = m2[c];
            }
            __syncthreads();
            // ---- adjoint of the over-relaxation and the primal step, per channel
            double gxb[C], gxn[C];   // (WEIGHTED: gxn holds h = r_c o gxn)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double gt = (sg1[c * PLANES + lj * S1 + li] - m1[c]) + (sg2[c * PLANES + lj * RI + li] - m2[c]);
                gxb[c] = sigma * gt;
                gxn[c] = gx[c] + opw * gxb[c];
                if constexpr (WEIGHTED) {
                    const double r = 1.0 / __builtin_fma(tau, w[c], 1.0);
                    gxn[c] = gxn[c] * r;
                }
                sxn[c * PLANES + l] = gxn[c];
            }
            __syncthreads();
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double h = gxn[c];
                    const double d1 = sxn[c * PLANES + n1] - h;
                    const double d2 = sxn[c * PLANES + n2] - h;
                    gf[c] += tau * (w[c] * h);
                    if (want_w) gw[c] += tau * ((f[c] - xp[c][s]) * h);
                    gy1[c] = gy1[c] - tau * d1;
                    gy2[c] = gy2[c] - tau * d2;
                    gx[c] = h - omega * gxb[c];
                }
            } else {
                const double tc = tau * cr;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double d1 = sxn[c * PLANES + n1] - gxn[c];
                    const double d2 = sxn[c * PLANES + n2] - gxn[c];
                    gf[c] += tc * gxn[c];
                    gy1[c] = gy1[c] - tc * d1;
                    gy2[c] = gy2[c] - tc * d2;
                    gx[c] = cr * gxn[c] - omega * gxb[c];
                }
            }
        }
    }

    if (core) {
        const size_t idx = base + qi + (size_t)M * qj;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __hip_atomic_store(&A.out[0][idx + c * npx], gx[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[1][idx + c * npx], gy1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.out[2][idx + c * npx], gy2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.gf[idx + c * npx], gf[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&A.ga[idx + c * npx], c == 0 ? ga : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (WEIGHTED)
                if (want_w) __hip_atomic_store(&A.gw[idx + c * npx], gw[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace bpltv
