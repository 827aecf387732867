/*
 * taped_oracle.c -- CPU restatement of the one-plane taped ("unrolled") TV family: forward with its tape, tangent sweep and
 * reverse sweep of the models tv, weighted, l1 and kl.  TEST INFRASTRUCTURE ONLY (as bpltv_oracle.c: tests/ may load it,
 * nothing under bpldenoising_amd/ does).
 *
 * Written from the header comment of bpldenoising_amd/csrc/tv_tile_kernels.hpp, operation for operation: every fma below is
 * one that comment writes, everything else is a plain IEEE operation (-ffp-contract=off, oracle/Makefile), sqrt and division
 * are the correctly rounded ones.  What the comment leaves to "G" and "G^T" -- the association of the four differences -- is
 * pdhg_x_pass's and pdhg_y_pass's of bpltv_oracle.c:
 *     (G^T y)(i,j) = (y1[i-1,j] - y1[i,j]) + (y2[i,j-1] - y2[i,j])      out of range -> 0; in the reverse sweep the duals of
 *                                                                       the last image row / column enter as 0 as well
 *     (G x)(i,j)   = (x[i+1,j] - x[i,j],  x[i,j+1] - x[i,j])            0 at i = M-1 / j = N-1
 * so the tv forward is bplo_pdhg with rho = 0 bit for bit, and the weighted forward with w == 1.0 is the same bits again
 * (tests/test_taped_oracle.py).
 *
 * Every degenerate case follows the comment's convention, in the forward, the tangent and the reverse alike:
 *     out = n2 > alpha^2                      a dual exactly on the ball is not projected, and passes its (co)tangent whole
 *     m > 0 ? f + copysign(m, d) : f          a threshold met exactly holds the pixel at f
 *     act = x+ != f || w == 0                 decided on the taped iterate, f and w alone; three-way sign(x+ - f)
 *     q = D > 0 ? x+ / D : 0                  a KL iterate clamped to exactly 0 where w f = 0 passes nothing
 * The tangent recomputes the primal with the forward's own code (one loop, below), so its decisions are the forward's; the
 * reverse decides on whatever tape it is given.
 *
 * Layout: column-major M x N x O as bpltv_oracle.c; alpha is a full M x N map; w has wstride 0 (one plane) or M*N (one per
 * image); the tape is [k][z1, z2 (, x+)][image][pixel], two components for tv and three otherwise; tab is a step table of
 * bplo_step_table_gamma (rows {tau, sigma, omega, 1/(1+tau), 1+omega}).
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define BPLO_API __attribute__((visibility("default")))

double bplo_rsqrt_nr(double n2);   /* bpltv_oracle.c: the Newton rsqrt of "spec v2" */

enum { TO_TV = 0, TO_WEIGHTED = 1, TO_L1 = 2, TO_KL = 3 };

/* Counters of one forward run, on the oracle's own values (pixel-iterations):
 *   0 (a)  m == 0 with w > 0                               L1: the threshold met exactly
 *   1 (b0) m == 0 with w == 0 in iteration 0               L1: a pixel without data whose d is exactly zero
 *   2 (b1) m == 0 with w == 0 after iteration 0
 *   3 (c)  n2 == alpha^2                                   a dual exactly on the ball
 *   4 (c0) n2 == alpha^2 in iteration 0
 *   5 (d)  n2 == 0 in a segment of at most 64 consecutive pixels of one image row (fixed j, i in [64 s, 64 s + 64)) in which
 *          another pixel is projected.  A proxy for "in a wave whose other lanes project" -- a kernel's wave is two 32-pixel
 *          rows of its tile, whose position depends on the plan --: the rsqrt of zero is computed beside a projecting lane by
 *          a kernel that does not branch per pixel, and has to be discarded
 *   6 (e)  x+ == 0                                         KL: the iterate clamped
 *   7 (f)  D == 0                                          KL: the tail's denominator fma(tau w, f, x+ x+)
 *   8 (g)  m > 0 but x+ == f after rounding                L1: let through by the forward, read as held by act
 *   9 (h)  x+ == f with w == 0 after iteration 0           L1: act by w == 0 alone
 */
#define TO_NCOUNT 10

static inline int to_nc(int model) { return model == TO_TV ? 2 : 3; }

/* One image: K iterations from x = f, y = 0, and beside them (df_on) the tangent from dx = df, dy = 0.  tape, cnt nullable. */
static int run_image(int model, int M, int N, const double *f, const double *al, const double *w, int K, const double *tab,
                     double *x, double *tape, size_t tape_iter_stride, size_t plane, long long *cnt, int tangent,
                     const double *df, const double *dal, const double *dw, double *dx)
{
    const size_t n = (size_t)M * N;
    double *buf = (double *)calloc(6 * n, sizeof(double));
    if (!buf) return 2;
    double *y1 = buf, *y2 = buf + n, *xb = buf + 2 * n, *dy1 = buf + 3 * n, *dy2 = buf + 4 * n, *dxb = buf + 5 * n;
    memcpy(x, f, n * sizeof(double));
    if (tangent)
        for (size_t k = 0; k < n; ++k) dx[k] = df ? df[k] : 0.0;
    for (int it = 0; it < K; ++it) {
        const double tau = tab[5 * it], sigma = tab[5 * it + 1], omega = tab[5 * it + 2];
        const double rtab = tab[5 * it + 3], opw = tab[5 * it + 4];
        /* ---- primal step and over-relaxation (and their tangent) */
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < M; ++i) {
                const size_t k = i + (size_t)M * j;
                const double y1m = (i > 0) ? y1[k - 1] : 0.0;
                const double y2m = (j > 0) ? y2[k - M] : 0.0;
                const double div = (y1m - y1[k]) + (y2m - y2[k]);
                const double xo = x[k], fk = f[k], wk = w ? w[k] : 1.0;
                double xn, r = rtab;
                if (model == TO_L1) {
                    const double v = fma(-tau, div, xo);
                    const double d = v - fk;
                    const double m = fabs(d) - tau * wk;
                    xn = (m > 0.0) ? fk + copysign(m, d) : fk;
                    if (cnt) {
                        if (m == 0.0) cnt[wk > 0.0 ? 0 : (it == 0 ? 1 : 2)]++;
                        if (m > 0.0 && xn == fk) cnt[8]++;
                        if (xn == fk && wk == 0.0 && it > 0) cnt[9]++;
                    }
                } else if (model == TO_KL) {
                    const double v = fma(-tau, div, xo);
                    const double t = tau * wk;
                    const double c = v - t;
                    const double g = t * fk;
                    const double s = sqrt(c * c + 4.0 * g);
                    xn = (c >= 0.0) ? 0.5 * (c + s) : (2.0 * g) / (s - c);
                    if (cnt) {
                        if (xn == 0.0) cnt[6]++;
                        if (!(fma(t, fk, xn * xn) > 0.0)) cnt[7]++;
                    }
                } else {
                    double t;
                    if (model == TO_WEIGHTED) {
                        t = fma(-wk, fk, div);
                        r = 1.0 / fma(tau, wk, 1.0);
                    } else {
                        t = div - fk;
                    }
                    xn = fma(-tau, t, xo) * r;
                }
                xb[k] = fma(-omega, xo, opw * xn);
                x[k] = xn;
                if (tangent) {
                    const double dy1m = (i > 0) ? dy1[k - 1] : 0.0;
                    const double dy2m = (j > 0) ? dy2[k - M] : 0.0;
                    const double ddiv = (dy1m - dy1[k]) + (dy2m - dy2[k]);
                    const double dfk = df ? df[k] : 0.0, dwk = dw ? dw[k] : 0.0, dxo = dx[k];
                    double dxn;
                    if (model == TO_L1) {
                        const double dv = dxo - tau * ddiv;
                        const int act = xn != fk || wk == 0.0;
                        const double sg = (xn > fk) ? 1.0 : ((xn < fk) ? -1.0 : 0.0);
                        dxn = act ? dv - tau * (sg * dwk) : dfk;
                    } else if (model == TO_KL) {
                        const double dv = dxo - tau * ddiv;
                        const double t = tau * wk;
                        const double D = fma(t, fk, xn * xn);
                        const double q = (D > 0.0) ? xn / D : 0.0;
                        dxn = q * (xn * dv + t * dfk + tau * ((fk - xn) * dwk));
                    } else {
                        double dt;
                        if (model == TO_WEIGHTED) dt = (ddiv - wk * dfk) - dwk * (fk - xn);
                        else dt = ddiv - dfk;
                        dxn = (dxo - tau * dt) * r;
                    }
                    dxb[k] = opw * dxn - omega * dxo;
                    dx[k] = dxn;
                }
            }
        /* ---- dual step, tape, projection (and its derivative) */
        double *tz = tape ? tape + tape_iter_stride * it : NULL;
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < M; ++i) {
                const size_t k = i + (size_t)M * j;
                const double d1 = (i < M - 1) ? xb[k + 1] - xb[k] : 0.0;
                const double d2 = (j < N - 1) ? xb[k + M] - xb[k] : 0.0;
                const double a = al[k];
                double z1 = fma(sigma, d1, y1[k]);
                double z2 = fma(sigma, d2, y2[k]);
                if (tz) {
                    tz[k] = z1;
                    tz[plane + k] = z2;
                    if (model != TO_TV) tz[2 * plane + k] = x[k];
                }
                double dz1 = 0.0, dz2 = 0.0;
                if (tangent) {
                    const double dd1 = (i < M - 1) ? dxb[k + 1] - dxb[k] : 0.0;
                    const double dd2 = (j < N - 1) ? dxb[k + M] - dxb[k] : 0.0;
                    dz1 = dy1[k] + sigma * dd1;
                    dz2 = dy2[k] + sigma * dd2;
                }
                const double n2 = fma(z2, z2, z1 * z1);
                const double a2 = a * a;
                if (cnt && n2 == a2) { cnt[3]++; if (it == 0) cnt[4]++; }
                if (n2 > a2) {
                    const double q = bplo_rsqrt_nr(n2);
                    const double v = a * q;
                    if (tangent) {
                        const double e1 = z1 * q, e2 = z2 * q;
                        const double dot = e1 * dz1 + e2 * dz2;
                        const double da = dal ? dal[k] : 0.0;
                        dz1 = da * e1 + v * (dz1 - e1 * dot);
                        dz2 = da * e2 + v * (dz2 - e2 * dot);
                    }
                    z1 = z1 * v;
                    z2 = z2 * v;
                }
                y1[k] = z1;
                y2[k] = z2;
                if (tangent) { dy1[k] = dz1; dy2[k] = dz2; }
            }
        if (cnt && tz) {   /* (d): on the taped duals of this iteration, row segment by row segment */
            for (int j = 0; j < N; ++j)
                for (int i0 = 0; i0 < M; i0 += 64) {
                    const int i1 = (i0 + 64 < M) ? i0 + 64 : M;
                    long long zero = 0, proj = 0;
                    for (int i = i0; i < i1; ++i) {
                        const size_t k = i + (size_t)M * j;
                        const double n2 = fma(tz[plane + k], tz[plane + k], tz[k] * tz[k]);
                        if (n2 == 0.0) zero++;
                        if (n2 > al[k] * al[k]) proj++;
                    }
                    if (proj) cnt[5] += zero;
                }
        }
    }
    free(buf);
    return 0;
}

static int taped_run(int model, int M, int N, int O, const double *f, const double *al, const double *w, size_t wstride, int K,
                     const double *tab, double *u, double *tape, long long *cnt, int tangent, const double *df, const double *dal,
                     const double *dw, double *du)
{
    if (model < TO_TV || model > TO_KL || M < 1 || N < 1 || O < 0 || K < 0 || !f || !al || !tab || !u) return 1;
    if ((model != TO_TV) != (w != NULL)) return 1;
    if (wstride != 0 && wstride != (size_t)M * N) return 1;
    if (cnt && !tape) return 1;   /* class (d) is counted on the tape */
    const size_t n = (size_t)M * N, plane = n * (size_t)O;
    if (cnt) memset(cnt, 0, TO_NCOUNT * sizeof(long long));
    for (int img = 0; img < O; ++img) {
        const int rc = run_image(model, M, N, f + n * img, al, w ? w + wstride * img : NULL, K, tab, u + n * img,
                                 tape ? tape + n * img : NULL, (size_t)to_nc(model) * plane, plane, cnt, tangent,
                                 df ? df + n * img : NULL, dal, dw ? dw + wstride * img : NULL, tangent ? du + n * img : NULL);
        if (rc) return rc;
    }
    return 0;
}

/* forward: u, the full tape (nullable) and the counters (nullable; they need the tape) */
BPLO_API int bplo_taped_forward(int model, int M, int N, int O, const double *f, const double *alpha_map, const double *w,
                                size_t wstride, int K, const double *tab, double *u, double *tape, long long *counters)
{
    return taped_run(model, M, N, O, f, alpha_map, w, wstride, K, tab, u, tape, counters, 0, NULL, NULL, NULL, NULL);
}

/* tangent: du and u for the directions df (O planes), dalpha_map (one map), dw (planes as w); any of them NULL: zero */
BPLO_API int bplo_taped_tangent(int model, int M, int N, int O, const double *f, const double *alpha_map, const double *w,
                                size_t wstride, int K, const double *tab, const double *df, const double *dalpha_map,
                                const double *dw, double *du, double *u)
{
    if (!du) return 1;
    return taped_run(model, M, N, O, f, alpha_map, w, wstride, K, tab, u, NULL, NULL, 1, df, dalpha_map, dw, du);
}

/* reverse: grad_f, and the per-pixel, per-image terms ga and gw (gw NULL for tv) of dL/dalpha and dL/dw, for the cotangent
 * gu = dL/du, over the K iterations of `tape`.  Decides on the tape, f and w alone. */
BPLO_API int bplo_taped_reverse(int model, int M, int N, int O, const double *tape, const double *f, const double *alpha_map,
                                const double *w, size_t wstride, int K, const double *tab, const double *gu, double *grad_f,
                                double *ga_out, double *gw_out)
{
    if (model < TO_TV || model > TO_KL || M < 1 || N < 1 || O < 0 || K < 0 || !tape || !f || !alpha_map || !tab || !gu ||
        !grad_f || !ga_out)
        return 1;
    if ((model != TO_TV) != (w != NULL) || (model != TO_TV) != (gw_out != NULL)) return 1;
    if (wstride != 0 && wstride != (size_t)M * N) return 1;
    const size_t n = (size_t)M * N, plane = n * (size_t)O;
    const int nc = to_nc(model);
    double *buf = (double *)malloc(7 * n * sizeof(double));
    if (!buf) return 2;
    double *gx = buf, *gy1 = buf + n, *gy2 = buf + 2 * n, *gz1 = buf + 3 * n, *gz2 = buf + 4 * n, *gxb = buf + 5 * n, *h = buf + 6 * n;
    for (int img = 0; img < O; ++img) {
        const double *fk = f + n * img, *wk = w ? w + wstride * img : NULL;
        double *gf = grad_f + n * img, *ga = ga_out + n * img, *gw = gw_out ? gw_out + n * img : NULL;
        for (size_t k = 0; k < n; ++k) {
            gx[k] = gu[n * img + k];
            gy1[k] = 0.0; gy2[k] = 0.0; gf[k] = 0.0; ga[k] = 0.0;
            if (gw) gw[k] = 0.0;
        }
        for (int it = K - 1; it >= 0; --it) {
            const double tau = tab[5 * it], sigma = tab[5 * it + 1], omega = tab[5 * it + 2];
            const double c = tab[5 * it + 3], opw = tab[5 * it + 4];
            const double *tz = tape + (size_t)nc * plane * it + n * img;
            /* ---- adjoint of the projection, on the taped dual */
            for (size_t k = 0; k < n; ++k) {
                const double z1 = tz[k], z2 = tz[plane + k], a = alpha_map[k];
                const double n2 = fma(z2, z2, z1 * z1);
                if (n2 > a * a) {
                    const double q = bplo_rsqrt_nr(n2);
                    const double e1 = z1 * q, e2 = z2 * q;
                    const double dot = e1 * gy1[k] + e2 * gy2[k];
                    const double v = a * q;
                    gz1[k] = v * (gy1[k] - e1 * dot);
                    gz2[k] = v * (gy2[k] - e2 * dot);
                    ga[k] += dot;
                } else {
                    gz1[k] = gy1[k];
                    gz2[k] = gy2[k];
                }
            }
            /* ---- adjoint of the over-relaxation and of the primal step's own value */
            for (int j = 0; j < N; ++j)
                for (int i = 0; i < M; ++i) {
                    const size_t k = i + (size_t)M * j;
                    const double a = (i < M - 1) ? gz1[k] : 0.0, am = (i > 0) ? gz1[k - 1] : 0.0;
                    const double b = (j < N - 1) ? gz2[k] : 0.0, bm = (j > 0) ? gz2[k - M] : 0.0;
                    const double gt = (am - a) + (bm - b);
                    gxb[k] = sigma * gt;
                    const double gxn = gx[k] + opw * gxb[k];
                    if (model == TO_TV) {
                        h[k] = gxn;
                        gf[k] += tau * c * gxn;
                        gx[k] = c * gxn - omega * gxb[k];
                    } else if (model == TO_WEIGHTED) {
                        const double r = 1.0 / fma(tau, wk[k], 1.0);
                        h[k] = gxn * r;
                        gf[k] += tau * (wk[k] * h[k]);
                        gw[k] += tau * ((fk[k] - tz[2 * plane + k]) * h[k]);
                        gx[k] = h[k] - omega * gxb[k];
                    } else if (model == TO_L1) {
                        const double xk = tz[2 * plane + k];
                        const int act = xk != fk[k] || wk[k] == 0.0;
                        const double sg = (xk > fk[k]) ? 1.0 : ((xk < fk[k]) ? -1.0 : 0.0);
                        h[k] = act ? gxn : 0.0;
                        gf[k] += act ? 0.0 : gxn;
                        gw[k] += -tau * (sg * h[k]);
                        gx[k] = h[k] - omega * gxb[k];
                    } else {
                        const double xk = tz[2 * plane + k];
                        const double t = tau * wk[k];
                        const double D = fma(t, fk[k], xk * xk);
                        const double q = (D > 0.0) ? xk / D : 0.0;
                        const double e = q * gxn;
                        h[k] = xk * e;
                        gf[k] += t * e;
                        gw[k] += tau * ((fk[k] - xk) * e);
                        gx[k] = h[k] - omega * gxb[k];
                    }
                }
            /* ---- gy = gz - tau (tv: tau c) G h */
            for (int j = 0; j < N; ++j)
                for (int i = 0; i < M; ++i) {
                    const size_t k = i + (size_t)M * j;
                    const double d1 = (i < M - 1) ? h[k + 1] - h[k] : 0.0;
                    const double d2 = (j < N - 1) ? h[k + M] - h[k] : 0.0;
                    if (model == TO_TV) {
                        gy1[k] = gz1[k] - tau * c * d1;
                        gy2[k] = gz2[k] - tau * c * d2;
                    } else {
                        gy1[k] = gz1[k] - tau * d1;
                        gy2[k] = gz2[k] - tau * d2;
                    }
                }
        }
        for (size_t k = 0; k < n; ++k) gf[k] = gf[k] + gx[k];
    }
    free(buf);
    return 0;
}

/* What the sweeps decide on a tape, with the sweeps' own expressions, per pixel and image (1.0 / 0.0):
 *   projected[k]  out = fma(z2, z2, z1*z1) > alpha^2 in at least one iteration (only then does ga receive anything)
 *   data[k]       the data step passes something into gw in at least one iteration: l1: x+ != f; kl: D = fma(tau w, f, x+ x+) > 0;
 *                 weighted: always; NULL for tv */
BPLO_API int bplo_taped_decisions(int model, int M, int N, int O, const double *tape, const double *f, const double *alpha_map,
                                  const double *w, size_t wstride, int K, const double *tab, double *projected, double *data)
{
    if (model < TO_TV || model > TO_KL || M < 1 || N < 1 || O < 0 || K < 0 || !tape || !f || !alpha_map || !tab || !projected) return 1;
    if ((model != TO_TV) != (w != NULL) || (model != TO_TV) != (data != NULL)) return 1;
    if (wstride != 0 && wstride != (size_t)M * N) return 1;
    const size_t n = (size_t)M * N, plane = n * (size_t)O;
    const int nc = to_nc(model);
    for (int img = 0; img < O; ++img)
        for (size_t k = 0; k < n; ++k) {
            const size_t q = n * img + k;
            double pr = 0.0, da = (model == TO_WEIGHTED) ? 1.0 : 0.0;
            for (int it = 0; it < K; ++it) {
                const double *tz = tape + (size_t)nc * plane * it + q;
                const double z1 = tz[0], z2 = tz[plane], a = alpha_map[k];
                if (fma(z2, z2, z1 * z1) > a * a) pr = 1.0;
                if (model == TO_L1 && tz[2 * plane] != f[q]) da = 1.0;
                if (model == TO_KL) {
                    const double xk = tz[2 * plane], t = tab[5 * it] * w[wstride * img + k];
                    if (fma(t, f[q], xk * xk) > 0.0) da = 1.0;
                }
            }
            projected[q] = pr;
            if (data) data[q] = da;
        }
    return 0;
}

BPLO_API int bplo_taped_ncounters(void) { return TO_NCOUNT; }
