// unrolled_kernels.hpp -- reverse mode through the PDHG iterations themselves (bpltv_unrolled_denoise / bpltv_unrolled_vjp,
// DESIGN.md section 4.6): the TV solve that records the dual before every projection, and the sweep that runs the recorded
// iterations backwards.  The reference has no counterpart: its gradients (/root/reference/src/TVLearningFunctionVec.jl:
// 98-135) differentiate the exact minimiser, not the iteration.
//
// Forward = "spec v2" of pdhg_tile_kernel<double, 1, 1, 32, 32> with rho = 0, operation for operation, so u is
// bpltv_denoise's bit for bit (tests/test_gpu_unrolled.py); in iteration k it also stores z_k = y_k + sigma_k G xbar_k.
// Reverse, per pixel, k = K-1 ... 0, from gx = dL/du, gy = gf = ga = 0 (-ffp-contract=off; fma only where written):
//     n2  = fma(z2, z2, z1*z1);  out = n2 > alpha^2                   (the forward's expression: the same decision)
//     out:  r = rsqrt_nr(n2); e = z*r; dot = e1*gy1 + e2*gy2; gz = (alpha*r)*(gy - e*dot); ga += dot
//     else: gz = gy
//     gxb = sigma_k * G^T gz;  gxn = gx + (1 + omega_k)*gxb;  c = 1/(1 + tau_k) (tabulated)
//     gf += tau_k*c*gxn;  gy = gz - tau_k*c * G gxn;  gx = c*gxn - omega_k*gxb
// and dL/df = gf + gx after the last step (x_0 = f, y_0 = 0).
//
// Tape layout (private): [k][component][image][pixel], so a wave's stores and loads run along i.
#pragma once
#include <hip/hip_runtime.h>

#include "pdhg_kernels.hpp"

namespace bpltv {

constexpr int UN_R = 32;        // region (core + halo) of one workgroup: 32 x 32 pixels, one per thread
constexpr int UN_REV_T = 8;     // most reverse iterations per launch: their taped duals sit in registers (2 * 8 doubles)
constexpr size_t unrolled_lds_bytes() { return pdhg_lds_bytes(UN_R, UN_R); }   // the dynamic planes; the step rows are static

struct UnrolledArgs {
    const double* xin;
    const double* y1in;
    const double* y2in;
    double* xout;
    double* y1out;
    double* y2out;
    const double* f;      // the dataset, O planes
    const double* alpha;  // am*an doubles, column major
    const double* tab;    // [maxiter][TAB_STRIDE]
    double* tape;         // [maxiter][2][O][M*N] (TAPE = false: not read)
    size_t plane;         // O * M*N: doubles of one tape component
    int am, an;
    int istride;          // doubles between per-image parameter blocks: 0 = one block for every image, am*an = image k reads block k
    int it0, nit;
    int tk0;              // tape base iteration: iteration k lives in slot k - tk0 (0: the full tape; a checkpointed sweep's
                          // segment tape starts at its segment's first iteration).  tab stays indexed by k itself
    int M, N;
    int halo;
    int first;            // 1: start from x = f, y = 0
    int img0;             // first image of this launch (grid.z = images of the launch chain)
};

// One workgroup per tile, grid (nTi, nTj, images), block 1024: weighted_tile_kernel's structure with the unweighted primal
// step, plus two stores per iteration of the pre-projection dual for the core pixels (valid in every iteration of a launch).
// TAPE = false: the same recurrence without those stores (the checkpoint pass of a checkpointed solve).
template <bool TAPE>
__global__ __launch_bounds__(UN_R * UN_R) void unrolled_tile_kernel(UnrolledArgs A) {
    constexpr int RI = UN_R, RJ = UN_R, S1 = RI + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char un_smem[];
    double* smem = reinterpret_cast<double*>(un_smem);
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
    // address and are zeroed afterwards (they stay 0).
    const int gi = min(oi + li, M - 1), gj = min(oj + lj, N - 1);
    const size_t pix = gi + (size_t)M * gj;
    size_t ai = (size_t)img * (size_t)A.istride;   // image img's block (the global image index: a launch chain starts at img0)
    if (amode == 2) {
        ai += pix;
    } else if (amode == 1) {
        const unsigned pa = ((unsigned)gi * (unsigned)A.am) / (unsigned)M;
        const unsigned pb = ((unsigned)gj * (unsigned)A.an) / (unsigned)N;
        ai += pa + (size_t)A.am * pb;
    }
    double x = 0.0, y1 = 0.0, y2 = 0.0;
    if (!first) {
        x = A.xin[base + pix];
        y1 = A.y1in[base + pix];
        y2 = A.y2in[base + pix];
    }
    double f = A.f[base + pix];
    double al = A.alpha[ai];
    const bool row_word = tid < A.nit * TAB_STRIDE;   // nit <= PDHG_MAX_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * A.it0 + tid];
    const bool in = (oi + li < M) && (oj + lj < N);
    if (first) { x = f; y1 = 0.0; y2 = 0.0; }
    if (!in) { f = 0.0; x = 0.0; y1 = 0.0; y2 = 0.0; al = 0.0; }
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
    const int qi = oi + li, qj = oj + lj;
    const bool core = qi >= ci0 && qi < ci1 && qj >= cj0 && qj < cj1;
    const size_t idx = base + qi + (size_t)M * qj;   // used by core pixels only
    double* tz = TAPE ? A.tape + (size_t)2 * A.plane * (A.it0 - A.tk0) + idx : nullptr;
    // halo rows do not need all the iterations (pdhg_tile_kernel): a wave owns two adjacent rows; core rows run them all
    int my_nit = nit;
    if (N > RJ) {
        const int r0 = (tid & ~63) / RI, r1 = min((tid | 63) / RI, RJ - 1);
        if (oj > 0) my_nit = min(my_nit, r1);
        if (oj + RJ < N) my_nit = min(my_nit, RJ - r0);
    }
    const int loop_nit = __builtin_amdgcn_readfirstlane(my_nit);
    double tau = srow[0], sigma = srow[1], omega = srow[2], inv1ptau = srow[3], opw = srow[4];
    for (int it = 0; it < loop_nit; ++it) {
        // ---- primal step: x <- prox_{tau * fidelity}(x - tau * G^T y); over-relaxation
        const double y1m = sy1[lj * S1 + li];
        const double y2m = sy2[lj * RI + li];
        const double div = (y1m - y1) + (y2m - y2);
        const double t = div - f;
        const double xo = x;
        const double xn = __builtin_fma(-tau, t, xo) * inv1ptau;
        const double b = __builtin_fma(-omega, xo, opw * xn);
        x = xn;
        sxb[l] = b;
        __syncthreads();
        const double* nrow = srow + TAB_STRIDE * ((it + 1 < nit) ? it + 1 : it);
        const double ntau = nrow[0], nsigma = nrow[1], nomega = nrow[2], ninv = nrow[3], nopw = nrow[4];
        // ---- dual step: y <- proj_{|y_ij| <= alpha_ij}(y + sigma * G xbar)
        const double d1 = sxb[n1] - b;
        const double d2 = sxb[n2] - b;
        double y1n = __builtin_fma(sigma, d1, y1);
        double y2n = __builtin_fma(sigma, d2, y2);
        if (TAPE) {
            if (core) {   // the tape: the dual before the projection
                __hip_atomic_store(tz, y1n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(tz + A.plane, y2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            tz += 2 * A.plane;
        }
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
        tau = ntau; sigma = nsigma; omega = nomega; inv1ptau = ninv; opw = nopw;
        __syncthreads();
    }
    for (int it = loop_nit; it < nit; ++it) {   // a spent halo wave: the two barriers of an iteration, nothing else
        __syncthreads();
        __syncthreads();
    }

    if (core) {
        // write-through stores, as pdhg_tile_kernel: the next launch reads this state from other XCDs
        __hip_atomic_store(&A.xout[idx], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.y1out[idx], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.y2out[idx], y2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct UnrolledRevArgs {
    const double* gxin;   // first: the cotangent dL/du
    const double* gy1in;
    const double* gy2in;
    double* gxout;
    double* gy1out;
    double* gy2out;
    double* gf;           // in place, owning core only
    double* ga;           // in place, owning core only: per-pixel parameter gradient
    const double* tape;   // [maxiter][2][O][M*N]
    const double* alpha;
    const double* tab;
    size_t plane;
    int am, an;
    int istride;          // as UnrolledArgs: 0, or am*an for one parameter block per image
    int khi, nit;         // this launch runs the iterations khi, khi - 1, ..., khi - nit + 1
    int tk0;              // tape base iteration, as UnrolledArgs (the launch stays inside the tape: khi - nit + 1 >= tk0)
    int M, N;
    int halo;
    int first;            // 1: start from gx = gxin, gy = gf = ga = 0
    int img0;
};

// The mirror image: same region, halo and tile_span, nit <= UN_REV_T reverse iterations per launch, each reaching one pixel
// in each axis.  gx, gy1, gy2 ping-pong between two state sets (neighbouring tiles read each other's halos); gf and ga are read
// and written by the owning core only.  gz1 goes through a plane with a zero guard column and gz2 through one with a zero
// guard row (G^T: neighbours i-1, j-1), gxn through the padded plane (G: neighbours i+1, j+1) -- the layouts of sy1, sy2,
// sxb.  Out-of-image lanes stay zero: the duals of the last image row / column enter the planes as 0, as G^T treats them.
__global__ __launch_bounds__(UN_R * UN_R) void unrolled_reverse_tile_kernel(UnrolledRevArgs A) {
    constexpr int RI = UN_R, RJ = UN_R, S1 = RI + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char un_smem[];
    double* smem = reinterpret_cast<double*>(un_smem);
    double* sg1 = smem;                              // [RJ][S1]
    double* sg2 = smem + RJ * S1;                    // [RJ+1][RI]
    double* sxn = smem + RJ * S1 + (RJ + 1) * RI;    // [RJ][RI] + RI + 1
    __shared__ __attribute__((aligned(16))) double srow[UN_REV_T * TAB_STRIDE];

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
    const int nit = A.nit;
    const int klo = A.khi - nit + 1;

    // ---- prologue: every global load, the launch's taped duals included, is issued before the first use
    const int gi = min(oi + li, M - 1), gj = min(oj + lj, N - 1);
    const size_t pix = gi + (size_t)M * gj;
    size_t ai = (size_t)img * (size_t)A.istride;   // image img's block (the global image index: a launch chain starts at img0)
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
    double gx = A.gxin[base + pix], gy1 = 0.0, gy2 = 0.0, gf = 0.0, ga = 0.0;
    if (!first) {
        gy1 = A.gy1in[base + pix];
        gy2 = A.gy2in[base + pix];
        if (core) {
            gf = A.gf[base + pix];
            ga = A.ga[base + pix];
        }
    }
    double al = A.alpha[ai];
    double z1[UN_REV_T], z2[UN_REV_T];   // z?[s]: iteration khi - s
    const double* tz = A.tape + (size_t)2 * A.plane * (A.khi - A.tk0) + base + pix;
#pragma unroll
    for (int s = 0; s < UN_REV_T; ++s) {
        z1[s] = 0.0; z2[s] = 0.0;
        if (s < nit) {
            z1[s] = tz[0];
            z2[s] = tz[A.plane];
        }
        tz -= 2 * A.plane;
    }
    const bool row_word = tid < nit * TAB_STRIDE;   // nit <= UN_REV_T: the host checks
    double row_w = 0.0;
    if (row_word) row_w = A.tab[(size_t)TAB_STRIDE * klo + tid];
    if (!in) { gx = 0.0; gy1 = 0.0; gy2 = 0.0; al = 0.0; }
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
    for (int s = 0; s < UN_REV_T; ++s) {
        if (s < nit) {   // (uniform)
            const double* row = srow + TAB_STRIDE * (nit - 1 - s);
            const double tau = row[0], sigma = row[1], omega = row[2], c = row[3], opw = row[4];
            // ---- adjoint of the projection, on the taped dual
            const double za = in ? z1[s] : 0.0, zb = in ? z2[s] : 0.0;
            const double nn = __builtin_fma(zb, zb, za * za);
            double gz1 = gy1, gz2 = gy2;
            if (nn > a2) {
                const double r = rsqrt_nr(nn);
                const double u1 = za * r, u2 = zb * r;
                const double dot = u1 * gy1 + u2 * gy2;
                const double v = al * r;
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

    if (core) {
        const size_t idx = base + qi + (size_t)M * qj;
        __hip_atomic_store(&A.gxout[idx], gx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.gy1out[idx], gy1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.gy2out[idx], gy2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.gf[idx], gf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.ga[idx], ga, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// dL/df = gf + gx after the last reverse step (x_0 = f)
__global__ __launch_bounds__(256) void unrolled_gradf_kernel(const double* __restrict__ gf, const double* __restrict__ gx, size_t n,
                                                             double* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[q] = gf[q] + gx[q];
}

}  // namespace bpltv
