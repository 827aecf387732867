/*
 * bpltv.h -- C ABI of libbpltv: the MI355X (gfx950) inner TV-denoising solver that drops in behind
 * BPLDenoising's evaluate/solve surface.
 *
 * What it replaces in the reference (dvillacis/BPLDenoising, all paths relative to its root):
 *   src/TVLearningFunctionVec.jl:14-27   tv_op_learning_function(x, data, D) -> (u, cost, grad)
 *   src/TVLearningFunctionVec.jl:45-70   denoise(data, x::Real|AbstractArray, op)
 *   src/BPLDenoising.jl:41-82            TVDenoise(data, parameter)          (maxiter = 10000)
 *   src/TVLearningFunctionVec.jl:72-254  gradient / gradient_reg (adjoint state, per image)
 * and, inside those, the external VariationalImaging.op_denoise_pdps loop they call
 * (src/TVLearningFunctionVec.jl:52,67).  The caller -- bilevel_learn, src/TRBox.jl:36,46,227 --
 * is untouched: it only sees a function (x, data, D) -> (u, cost, grad).
 *
 * Conventions
 *   - Plain C: pointers and sizes only.  Every function returns 0 on success or a BPLTV_E_* code;
 *     bpltv_last_error() gives the message.  Nothing throws, prints, or exits.
 *   - Images are Julia `Array{Float64,3}` of size (M, N, O), column major: element (i, j, k) at
 *     i + M*j + M*N*k.  data[1] = ubar (ground truth), data[2] = f (noisy), src/TVLearningFunctionVec.jl:15-16.
 *   - The parameter x is passed as (alpha, am, an), column major am x an:
 *        1 x 1  scalar alpha;  m x n patch parameter (upsampled piecewise-constant, PatchOp);
 *        M x N  per-pixel map.   grad has the same shape (src/TRBox.jl:37-39,167,237).
 *   - Host pointers are read/written during the call only; the library keeps no host pointer.
 *     One call in flight per handle; calls block until the device work is complete.  Any number of handles may be
 *     alive; the handles of one device share its streams (a second handle runs at the speed of the first), so handles
 *     of the SAME device driven from different host threads at once are serialised on the device, not concurrent.
 *   - bpltv_create drives one GPU.  bpltv_create_multi drives several from ONE host thread (the single
 *     Julia task of src/TRBox.jl:192-273): images block-sharded over the devices, one worker thread and
 *     stream per device inside the library, one RCCL collective over xGMI per evaluation on the
 *     [cost, grad...] vector; every other entry point takes either kind of handle.  A host that prefers
 *     one process per GPU shards the images itself and all-reduces bpltv_evaluate_partial /
 *     bpltv_evaluate_device (bpltv_per_image for sharding-independent sums); see INTEGRATION.md.
 */
#ifndef BPLTV_H
#define BPLTV_H

#ifdef __cplusplus
extern "C" {
#endif

#define BPLTV_VERSION 4

enum {
    BPLTV_OK = 0,
    BPLTV_E_ARG = 1,      /* bad argument (null pointer, size mismatch, unsupported shape)   */
    BPLTV_E_HIP = 2,      /* HIP runtime error (message holds hipGetErrorString)             */
    BPLTV_E_NODATA = 3,   /* evaluate/denoise before set_data                                */
    BPLTV_E_NUMERIC = 4,  /* adjoint factorisation broke down (non-positive pivot)           */
    BPLTV_E_NOMEM = 5,
    BPLTV_E_UNSUPPORTED = 6
};
/* Sizes: PDHG, loss, sweep and the adjoint gradient accept any M x N x O whose images fit in HBM.  The gradient
 * factors its linear system by a nested-dissection (multifrontal) Cholesky (about 0.9 KB of workspace per pixel:
 * 0.94 GB for a 1024 x 1024 image); when the workspace of all O images does not fit it runs in groups of as many
 * images as fit, with bitwise the same result (stats.adjoint_chunks; bpltv_set_option "adjoint_budget_mb" forces a budget).
 * params.reserved[4] selects the cross-check solvers: banded Cholesky (LDS window for M <= 138, HBM-resident band
 * of M*N*(M+1) doubles per image beyond; whole batch at once) or block cyclic reduction (M <= 128).  All workspaces
 * are allocated on first use and released again if an allocation fails. */

typedef struct bpltv_handle bpltv_t;

/* The solver NamedTuple of src/TVLearningFunctionVec.jl:33-43 (+ the learning function's Dt). */
typedef struct bpltv_params {
    double rho;          /* Huber smoothing of the TV term; reference 0                           */
    double tau0;         /* reference 5                                                           */
    double sigma0;       /* reference 0.99/5                                                      */
    int accel;           /* reference true                                                        */
    int maxiter;         /* reference 5000 (TVDenoise: 10000); fixed count, no early stop         */
    double delta_t;      /* reference 1e-6: D > delta_t -> gradient, else gradient_reg            */
    int check_every;     /* > 0: evaluate the duality gap every check_every iterations            */
    double gap_tol;      /* > 0 with check_every > 0: stop once max-image gap <= gap_tol.
                            0 = reference behaviour (always maxiter iterations)                   */
    int tile_iters;      /* PDHG iterations fused per kernel launch (temporal blocking depth);
                            0 = library default for the image size                                */
    int use_graph;       /* 1 (default): replay the launch sequence from a hipGraph               */
    double kappa_cap;    /* cap on the active-set weight 1/eps() of the adjoint system; 0 = 1e14  */
    int refine;          /* iterative-refinement sweeps of the adjoint solve; < 0 = default: 4 / 1 / 0 for the
                            scalar gradient / patch and pixel-map parameters / gradient_reg with nested
                            dissection and the HBM band, 3 / 2 / 2 with block cyclic reduction and the
                            LDS band (bpltv_weighted_vjp included); the sum of regularisers: 5, and 1 for
                            gradient_reg, on every factorisation                                      */
    int deterministic;   /* multi-GPU handles, scalar / patch parameters: 1 = all-gather the per-image rows
                            [cost_k, grad_k...] and add them in global image order, so that cost and grad are
                            bitwise the same for every number of GPUs (and equal to a single handle's);
                            0 (default) = one all-reduce(sum) of the per-device partial vectors           */
    int reserved[5];     /* tuning / measurement knobs, 0 = default:
                            [0] PDHG kernel variant (1-based index into the variant table of bpltv.hip; sum of
                                regularisers: 1 = 32x32 region / 1 px per thread, 2 = 48x48 / 3 px per thread)
                            [1] number of independent launch chains (image groups replayed concurrently)
                            [2] 1 = replay those chains one after the other (isolated kernel timing)
                            [3] must be 0 (BPLTV_E_ARG otherwise); timing-experiment switches exist only in
                                tools/ builds compiled with -DBPLTV_EXPERIMENTS
                            [4] adjoint factorisation: 0 automatic, 1 banded Cholesky, 2 block cyclic reduction
                                (M <= 128, N >= 2; BPLTV_E_UNSUPPORTED otherwise), 3 nested-dissection
                                (multifrontal) Cholesky                                             */
    /* The three choices of the PDHG recurrence that the reference does not pin (its loop, op_denoise_pdps, lives
     * in the absent package VariationalImaging: src/TVLearningFunctionVec.jl:33-43,52).  0
     * everywhere = the restatement every parity claim refers to.  A user who has VariationalImaging on disk and
     * finds it differs aligns the library with these fields instead of rebuilding it.  TV model, dtype 64. */
    int init;            /* 0: x0 = f (default); 1: x0 = 0                                         */
    int order;           /* 0: primal step first (default); 1: dual step first (y from xbar of the previous
                            iteration, then x, then the over-relaxation)                           */
    double opnorm;       /* operator-norm estimate L dividing tau0 and sigma0; 0 = sqrt(8) (sum of
                            regularisers: sqrt(18)), e.g. 2*sqrt(2)*(1 - 1/n) for a tighter bound   */
} bpltv_params;

typedef struct bpltv_stats {
    int M, N, O, device;
    int iterations;            /* PDHG iterations executed by the last denoise/evaluate          */
    int launches;              /* PDHG kernel launches of that call                               */
    int tile_iters;            /* fused iterations per launch actually used                       */
    int tiles;                 /* workgroups per PDHG launch                                      */
    int region_i, region_j;    /* pixels one workgroup computes per fused iteration (core + halo): with tiles
                                  and tile_iters this gives the redundancy of the temporal blocking         */
    int graph_used;
    double pdhg_ms;            /* HIP-event time of the PDHG launch sequence (device)            */
    double cost_ms;
    double adjoint_ms;         /* HIP-event time of the adjoint gradient (all images)            */
    double total_ms;           /* host wall time of the last call                                 */
    double bytes_per_px_iter;  /* algorithmic bytes: 56 (scalar/patch alpha) or 64 (alpha map)    */
    double algorithmic_bytes;  /* bytes_per_px_iter * M*N*O * iterations                          */
    double last_gap;           /* max over images of the duality gap if it was computed, else -1  */
    double adjoint_residual;   /* max over images of ||D^-1/2 (rhs - A p)|| / ||D^-1/2 rhs||, D = diag(A), after
                                  refinement, over the rows that do not carry the active-set weight (a constant
                                  image has none and reports 0): the quality gate of the adjoint solve (<= 1e-8 on
                                  a correct solve; above BPLTV_RESIDUAL_GATE the call fails with BPLTV_E_NUMERIC) */
    double adjoint_residual_raw; /* the same without the diagonal scaling: dominated by the rounding of
                                  the 1e14-weighted active rows, informational only                   */
    double kappa_used;         /* active-set weight of the adjoint system that produced the returned
                                  gradient: 1/eps() capped by kappa_cap (scalar), 1/sqrt(eps()) (patch),
                                  times 1e-2 per retry; 0 for gradient_reg                             */
    int adjoint_attempts;      /* factorisations tried by the last gradient: 1 = no breakdown, 2..3 = the
                                  weight was reduced by 1e-2 per retry after a non-positive pivot or a
                                  residual above the gate                                              */
    int adjoint_method;        /* 1 banded Cholesky (LDS window), 2 block cyclic reduction,
                                  3 banded Cholesky (HBM band), 4 banded LU (sum of regularisers, row-scaled
                                  gradient_reg system, with reserved[4] = 1), 5 nested-dissection (multifrontal)
                                  Cholesky, 6 nested-dissection LU (that row-scaled system, the default),
                                  7 reverse sweep over the taped iterations (bpltv_unrolled_vjp),
                                  8 tangent sweep through the iterations (bpltv_unrolled_jvp),
                                  9 reverse sweep over the taped weighted iterations (bpltv_weighted_unrolled_vjp),
                                  10 reverse sweep over the taped sum-of-regularisers iterations (bpltv_sumregs_unrolled_vjp),
                                  11 tangent sweep through the weighted iterations (bpltv_weighted_unrolled_jvp),
                                  12 reverse sweep over the taped channel-coupled iterations (bpltv_color_unrolled_vjp),
                                  13 tangent sweep through the channel-coupled iterations (bpltv_color_unrolled_jvp),
                                  14 reverse sweep over the taped weighted channel-coupled iterations
                                  (bpltv_color_weighted_unrolled_vjp),
                                  15 reverse sweep over the taped TV-L1 iterations (bpltv_lone_unrolled_vjp),
                                  16 reverse sweep over the taped TV-KL iterations (bpltv_kl_unrolled_vjp),
                                  17 tangent sweep through the TV-L1 iterations (bpltv_lone_unrolled_jvp),
                                  18 tangent sweep through the TV-KL iterations (bpltv_kl_unrolled_jvp) */
    int reg_gradient_used;     /* 1 if the last evaluate took the gradient_reg branch             */
    int ngpus;                 /* distinct devices behind this handle (1 for bpltv_create)        */
    int shards;                /* image shards (= worker threads) behind this handle              */
    int collective;            /* last evaluate of a multi handle: 0 none (one shard), 1 ncclAllReduce,
                                  2 ncclAllGather + ordered sum, 3 host sum (repeated devices)     */
    double collective_ms;      /* host wall time of that collective (launch + completion)        */
    int nccl_ranks;            /* ranks of the RCCL communicator behind a multi handle as RCCL itself reports them
                                  (ncclCommCount); 0 = no communicator (single-device handle, repeated devices)  */
    int hb_sync;               /* cross-stream dependencies of the HBM band pipeline used by the last gradient:
                                  0 not used, 1 HIP events, 2 stream memory operations (hipStreamWaitValue32)    */
    int adjoint_chunks;        /* image groups the last adjoint gradient was processed in (1 = whole batch at once;
                                  more when the factor workspace of all images does not fit, option "adjoint_budget_mb") */
    int pdhg_variant;          /* 1-based index of the PDHG kernel the last solve ran (the variant table of
                                  csrc/bpltv.hip: 1..15 pdhg_tile_kernel, 16..18 pdhg_wave_kernel, 19.. pdhg_rows_kernel and its re-cuts;
                                  sum of regularisers: 1 sr_tile_kernel, 2 sr_strip_kernel)                      */
    int ncu;                   /* compute units of the device (hipDeviceProp_t.multiProcessorCount): what bench.py prices
                                  the VALU issue floor against                                                   */
    int launch_chains;         /* independent launch chains (image groups replayed concurrently) of the last solve */
    int sweep_shards;          /* last (sumregs_)sweep of a multi handle: devices the K parameter blocks were split over
                                  (replica mode), 0 = the images were split / single device                        */
    int sweep_groups;          /* last bpltv_sumregs_sweep: groups of parameter blocks it ran in (1 = all K at once; more
                                  beyond 65535 problems or when the state does not fit, option "sr_sweep_budget_mb") */
    double launch_host_ms[2];  /* host time the last solve's hipGraphLaunch calls took: chain 0 (calling thread) and
                                  chain 1 (launcher thread); 0 when the solve had one chain or ran without graphs    */
} bpltv_stats_t;

#define BPLTV_RESIDUAL_GATE 1e-6

/* Fill *p with the reference defaults (src/TVLearningFunctionVec.jl:33-43, delta_t 1e-6). */
int bpltv_default_params(bpltv_params *p);

/* Create a solver for O images of size M x N on HIP device `device` (-1 = current device).
 * dtype: 64 = Float64, the reference's arithmetic (src/TVLearningFunctionVec.jl:8-9) and what every parity claim
 * refers to.  32 = opt-in: the PDHG iteration of the TV model (bpltv_denoise, bpltv_evaluate, bpltv_sweep) runs in
 * single precision -- f, the parameter and the step table rounded to float, state in float, half the bytes per
 * pixel-iteration -- and its result is widened to double; loss, duality gap, adjoint gradient, the sum-of-regularisers
 * model and every array crossing this boundary stay Float64.  Narrower than the reference: u differs from the
 * Float64 result by up to ~2e-5 absolute after 5000 iterations, and the gradient by ~1 %: the reference's active set
 * |grad u| < 1e-12 (src/TVLearningFunctionVec.jl:110) does not survive float noise in u (tests/test_gpu_f32.py).  Other values: BPLTV_E_ARG. */
int bpltv_create(bpltv_t **h, int M, int N, int O, int device, int dtype);
/* The same over `ngpus` devices (0 = all visible; devices 0..ngpus-1) driven from one host thread -- the
 * form SURVEY section 8(b)/(e) specifies for the single Julia task of src/TRBox.jl:192-273.  Images
 * [lo_k, hi_k) = block distribution of O over min(ngpus, O) shards (the first O % shards get one more);
 * communicator from ncclCommInitAll; per evaluation ONE RCCL collective on [cost, grad...] (1 + am*an
 * doubles): ncclAllReduce(sum, f64), or ncclAllGather of the per-image rows when params.deterministic.
 * set_data / denoise / evaluate / gradient / sweep / per_image / duality_gap take and return whole-batch
 * host arrays exactly as with bpltv_create (each device copies its slice); the device-pointer entry points
 * (set_data_device, evaluate_device, u_device, copy_u_device) return BPLTV_E_UNSUPPORTED on more than one shard.
 * Status: verified with ngpus = 1 (a one-rank communicator) and with several shards on one device (host sum); the
 * collectives over ngpus > 1 have not yet run on hardware -- tests/test_gpu_multi.py holds the checks that switch on
 * when two or more devices are visible.  stats.nccl_ranks reports what ncclCommCount says.
 * Devices beyond min(ngpus, O) hold no image shard (one image cannot be split), but bpltv_sweep uses them: see there. */
int bpltv_create_multi(bpltv_t **h, int M, int N, int O, int ngpus, int dtype);
/* Explicit placement: shard k of `nshards` runs on HIP device devices[k].  A device may appear more than
 * once (rehearsal of the sharded path on one GPU); RCCL cannot put two ranks on one device, so the collective
 * is then replaced by the same sum / ordered sum on the host. */
int bpltv_create_sharded(bpltv_t **h, int M, int N, int O, const int *devices, int nshards, int dtype);
int bpltv_destroy(bpltv_t *h);

/* Upload the dataset (ubar, f) once; it is identical for every evaluation of a run
 * (src/TRBox.jl:210,227 pass the same `ds`).  Host pointers. */
int bpltv_set_data(bpltv_t *h, const double *ubar, const double *f);
/* Same, from buffers already resident in HBM (device pointers, copied device-to-device). */
int bpltv_set_data_device(bpltv_t *h, const double *d_ubar, const double *d_f);

/* denoise(data, x, op; kwargs...): src/TVLearningFunctionVec.jl:45-70, src/BPLDenoising.jl:41-82.
 * u_out: host, M*N*O doubles, or NULL to leave the result on the device (bpltv_u_device). */
int bpltv_denoise(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p,
                  double *u_out);

/* The same solve with the parameter already resident in HBM (d_alpha: device pointer, am*an doubles, column major) and
 * the result left there (bpltv_u_device): no host array crosses the boundary, which is how bench.py times a pixel-map
 * parameter (8 MiB for 1024 x 1024) without a PCIe copy in the timed region.  The entries are checked on the device
 * (finite, >= 0) exactly as bpltv_denoise checks a host array, before anything of the handle changes: a parameter
 * rejected with BPLTV_E_ARG leaves the handle as it was (its resident parameter, and so bpltv_duality_gap of the last
 * solve).  Single-device handles (multi: BPLTV_E_UNSUPPORTED beyond one shard). */
int bpltv_denoise_device(bpltv_t *h, const double *d_alpha, int am, int an, const bpltv_params *p);

/* tv_op_learning_function(x, data, D): src/TVLearningFunctionVec.jl:14-27.
 * cost_out: 1 double; grad_out: am*an doubles; u_out: host M*N*O doubles or NULL. */
int bpltv_evaluate(bpltv_t *h, const double *alpha, int am, int an, double delta,
                   const bpltv_params *p, double *u_out, double *cost_out, double *grad_out);

/* Sum-of-regularisers model: min_u 0.5||u - f||^2 + a1 ||G_fwd u|| + a2 ||G_bwd u|| + a3 ||G_ctr u|| (isotropic
 * 2,1 norms; forward, backward and centred differences), src/SumRegsLearningFunction.jl.
 *   bpltv_sumregs_evaluate = sumregs_learning_function(x, data, D; Dt = 1e-3) -> (u, cost, grad)   (:8-36)
 *   bpltv_sumregs_denoise  = sumregs_denoise(data, x, op1, op2, op3[, pOp])                       (:38-85)
 * alpha: 3 * am * an doubles, the three parameter slices x[:, :, k] (column major am x an) one after the other;
 * am = an = 1 is the Vector x = [a1; a2; a3] (:8), m x n x 3 the patch parameter (:22).  grad_out has the same
 * layout.  p = NULL: bpltv_sumregs_default_params (delta_t = 1e-3).  D > delta_t: sumregs_gradient (:264-407),
 * else sumregs_gradient_reg (:112-262; with a patch parameter its row-scaled system is not symmetric and is
 * factored by a banded LU).  The adjoint system is a 13-point stencil, factored by nested dissection (separators two
 * pixels wide; params.reserved[4] = 1: the HBM band solver at bandwidth 2M).
 * Both take single- and multi-device handles; set_data, per_image, u_device, duality_gap, stats are shared with the TV
 * model.  One block of 3 * am * an doubles per image instead of one for the batch: bpltv_sumregs_denoise_each and
 * bpltv_sumregs_vjp_each below. */
int bpltv_sumregs_default_params(bpltv_params *p);
int bpltv_sumregs_denoise(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_sumregs_evaluate(bpltv_t *h, const double *alpha, int am, int an, double delta, const bpltv_params *p,
                           double *u_out, double *cost_out, double *grad_out);
/* bpltv_sumregs_denoise with the parameter already resident in HBM (d_alpha: device pointer, 3*am*an doubles in the
 * layout above) and the result left there (bpltv_u_device / bpltv_copy_u_device), as bpltv_denoise_device is for the
 * TV model.  The entries are checked on the device (finite, >= 0; > 0 when params.rho != 0) before anything of the
 * handle changes: a rejected parameter returns BPLTV_E_ARG and leaves the handle, its last result and
 * bpltv_duality_gap as they were.  Single-device handles (multi: BPLTV_E_UNSUPPORTED beyond one shard). */
int bpltv_sumregs_denoise_device(bpltv_t *h, const double *d_alpha, int am, int an, const bpltv_params *p);

/* Sharded form: this handle's images only.  partial_out (host, 1 + am*an doubles) receives
 * [cost, grad...] summed over the handle's O images; the caller all-reduces it across shards
 * (cost and grad are plain sums over images: src/TVLearningFunctionVec.jl:20,80,172). */
int bpltv_evaluate_partial(bpltv_t *h, const double *alpha, int am, int an, double delta,
                           const bpltv_params *p, double *u_out, double *partial_out);
/* Same with the partial vector written to device memory (d_partial: 1 + am*an doubles in HBM),
 * ready for an RCCL all-reduce without a host round trip. */
int bpltv_evaluate_device(bpltv_t *h, const double *alpha, int am, int an, double delta,
                          const bpltv_params *p, double *d_partial);

/* Per-image pieces of the last evaluate (scalar or patch parameter; BPLTV_E_UNSUPPORTED for a pixel map):
 * out (host, O*(1 + am*an) doubles), image k at out + k*(1 + am*an): [cost_k, grad_k...].  The totals of
 * evaluate are these rows added in image order, so a host that gathers the rows of all shards and adds
 * them in global image order gets results that do not depend on how the images were sharded. */
int bpltv_per_image(bpltv_t *h, double *out);

/* Device pointer of the last primal result u (M*N*O doubles, valid until the next call). */
int bpltv_u_device(bpltv_t *h, const double **d_u);
/* Copy the last primal result to a device buffer owned by the caller. */
int bpltv_copy_u_device(bpltv_t *h, double *d_dst);

/* Duality gap of the last solve per image (host, O doubles): gap_k >= 0.5*||u_k - u*_k||^2.  TV model and
 * sum-of-regularisers model (the gap of whichever was solved last). */
int bpltv_duality_gap(bpltv_t *h, double *gap_out);

/* FwdGradientOp and its adjoint on the device (src/TVLearningFunctionVec.jl:17; matrix form
 * :106).  Host pointers, one M x N image; d1/d2 are the two stacked components. */
int bpltv_grad_fwd(bpltv_t *h, const double *x, double *d1, double *d2);
int bpltv_grad_fwd_adjoint(bpltv_t *h, const double *y1, const double *y2, double *out);

/* Adjoint gradient alone for given (u, ubar) held by the caller (host, M*N*O each):
 * gradient (reg = 0, src/TVLearningFunctionVec.jl:98-135,219-254) or gradient_reg (reg = 1,
 * :137-161,192-215), summed over the O images as the batch wrappers do (:72-96,163-190). */
int bpltv_gradient(bpltv_t *h, const double *u, const double *ubar, const double *alpha, int am,
                   int an, int reg, const bpltv_params *p, double *grad_out);

/* Vector-Jacobian product of u = denoise(f, alpha) for a cotangent gu = dL/du of any loss L: the adjoint system of
 * bpltv_gradient with gu in place of u - ubar (reg = 0), or -gu (reg = 1, divided by sqrt(alpha) for an array
 * parameter), solved once for the adjoint state p.  grad_f_out = p (reg = 0) or -p (reg = 1), p = S q the physical
 * adjoint state; grad_alpha_out = the parameter gradient of bpltv_gradient computed from the same p.  So gu = u - ubar
 * gives bitwise the grad_out of bpltv_gradient(u, ubar, ...).  With reg = 1 and an array parameter the reference's
 * system is not symmetric and its gradient uses M^-1, not M^-T: both outputs follow it.
 * u, gu, grad_f_out: host, M*N*O doubles; alpha, grad_alpha_out: am*an doubles.  Either output may be NULL, not
 * both.  The dataset is not used (no set_data needed).  alpha is checked as bpltv_denoise checks it (finite, >= 0;
 * > 0 for reg = 1 with an array parameter), gu must be finite: a rejected call returns BPLTV_E_ARG and leaves the handle
 * as it was.  The parameter is staged apart from the last solve's: bpltv_u_device, bpltv_duality_gap and the next
 * denoise are unchanged by a VJP (bpltv_per_image is not, as after bpltv_gradient).  The residual gate and the
 * kappa retry apply as in bpltv_gradient; stats report the adjoint (adjoint_ms, adjoint_residual, adjoint_method,
 * adjoint_chunks, kappa_used, reg_gradient_used).  dtype = 32 handles too (the adjoint is Float64 there as well).
 * Multi-device handles split the images as bpltv_gradient does: grad_f_out slices are written in place, grad_alpha_out
 * is the sum of the shards' in shard order. */
int bpltv_vjp(bpltv_t *h, const double *u, const double *alpha, int am, int an, int reg, const bpltv_params *p,
              const double *gu, double *grad_f_out, double *grad_alpha_out);
/* The same with every array in HBM (device pointers; e.g. torch tensors' .data_ptr()); the outputs are written there.
 * The parameter and the cotangent are checked on the device.  Single-device handles (multi: BPLTV_E_UNSUPPORTED
 * beyond one shard). */
int bpltv_vjp_device(bpltv_t *h, const double *d_u, const double *d_alpha, int am, int an, int reg,
                     const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha);

/* One parameter per image: the solves and vector-Jacobian products above for a batch whose O images each have their
 * own parameter -- what a network that predicts alpha per sample produces.  alphas: O blocks of am x an doubles, each
 * column major, block k at alphas + k*am*an, with bpltv_denoise's shape rules (1 x 1 scalar, m x n patch, M x N map).
 * u_k is bitwise what a one-image handle returns for (f_k, alpha_k).  Each function keeps the contract of its twin
 * (bpltv_denoise, bpltv_denoise_device, bpltv_vjp, bpltv_vjp_device): every entry is checked (finite, >= 0; > 0 when
 * params.rho != 0, and for reg = 1 with a patch or map parameter) before anything of the handle changes; dtype = 32
 * handles solve in float (the adjoint stays Float64); check_every / gap_tol and bpltv_duality_gap use image k's own
 * block; bpltv_u_device and bpltv_copy_u_device return the result; the VJP leaves the last solve untouched.
 * grad_f_out is bpltv_vjp's; grad_alphas_out receives O blocks, block k = image k's term alone (not summed over the
 * images: their sum in image order is bitwise bpltv_vjp's grad_alpha_out when all blocks are equal).  Multi-device
 * handles hand shard k the blocks [lo_k, hi_k); the device forms return BPLTV_E_UNSUPPORTED beyond one shard. */
int bpltv_denoise_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_denoise_each_device(bpltv_t *h, const double *d_alphas, int am, int an, const bpltv_params *p);
int bpltv_vjp_each(bpltv_t *h, const double *u, const double *alphas, int am, int an, int reg, const bpltv_params *p,
                   const double *gu, double *grad_f_out, double *grad_alphas_out);
int bpltv_vjp_each_device(bpltv_t *h, const double *d_u, const double *d_alphas, int am, int an, int reg,
                          const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alphas);

/* Per-pixel data-fidelity weight: the TV model with the data term weighted pixel by pixel,
 *     min_u 0.5 sum_ij w_ij (u_ij - f_ij)^2 + sum_ij alpha_ij |(grad u)_ij|,
 * for masks (w in {0, 1}: the solve inpaints where w = 0), a known noise variance per pixel (w = 1 / sigma^2) or a learnable
 * fidelity map.  The reference has no counterpart; its denoise is w == 1, and with w == 1 the result is
 * bpltv_denoise's bit for bit.  f is the resident dataset (bpltv_set_data).  w: wo planes of M*N doubles in the layout of f,
 * wo = 1 (one plane for every image) or wo = O (one per image), anything else BPLTV_E_ARG; every entry finite and >= 0.
 * alpha, am, an: as bpltv_denoise.  The acceleration uses gamma = the smallest entry of ALL of w (gamma = 0, e.g. a mask: the
 * unaccelerated iteration).  params: opnorm, tau0, sigma0, accel, maxiter, tile_iters and use_graph apply; rho, init and order
 * must be 0 (BPLTV_E_UNSUPPORTED); check_every / gap_tol are ignored (always maxiter iterations, as the sweeps).  The solve runs
 * in Float64 on dtype = 32 handles too.  w and alpha are checked (on the host) before anything of the handle changes: a rejected
 * call leaves the last solve and bpltv_duality_gap as they were.  The solve becomes the handle's last solve: bpltv_u_device /
 * bpltv_copy_u_device return its u, bpltv_duality_gap its gap
 *     0.5 sum w (u - f)^2 + sum alpha |grad u| - sum (d f - d^2 / (2 w)),  d = grad^T y,   >= 0.5 sum w (u - u*)^2
 * (BPLTV_E_UNSUPPORTED when gamma = 0: the dual objective divides by w).  A weighted and an unweighted solve on one handle never
 * replay each other's captured graphs.  stats: iterations, launches, tile_iters, tiles, pdhg_ms, total_ms; bytes_per_px_iter = 64
 * (scalar / patch parameter) or 72 (map); pdhg_variant = 0.  u_out: host, M*N*O doubles, or NULL.  Multi-device handles over
 * more than one shard: BPLTV_E_UNSUPPORTED (all four functions). */
int bpltv_weighted_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                           const bpltv_params *p, double *u_out);
/* The same with w and the parameter already resident in HBM (device pointers) and the result left there (bpltv_u_device);
 * both are checked on the device, before anything of the handle changes. */
int bpltv_weighted_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                  const bpltv_params *p);
/* Vector-Jacobian product of u = weighted_denoise(f, alpha, w) for a cotangent gu = dL/du, in the reference's `gradient`
 * linearisation (bpltv_vjp's reg = 0: active set |grad u| < 1e-12 with the kappa weight and its retry).  With
 * A = diag(w) + K, K the matrix bpltv_vjp builds from (u, alpha), one solve A p = gu gives
 *     grad_f_out = w o p,     grad_w_out = -(u - f) o p,     grad_alpha_out = bpltv_vjp's parameter gradient with this p.
 * The system is solved in the node-scaled form (I + S K S) q = S gu, S = diag(w)^-1/2, p = S q, which needs every w > 0
 * (BPLTV_E_ARG otherwise); with w == 1, grad_f_out and grad_alpha_out are bitwise bpltv_vjp's.  u, gu, grad_f_out: M*N*O
 * doubles; w as above; grad_w_out: M*N*wo doubles, for wo = 1 the sum over the images in image order; alpha, grad_alpha_out:
 * am*an doubles.  Any output may be NULL, not all three; f (M*N*O doubles) may be NULL only if grad_w_out is (BPLTV_E_ARG
 * otherwise).  No dataset is needed.  gu must be finite.  Every rejection comes before anything of the handle changes; w and
 * the parameter are staged apart, so the last solve, bpltv_u_device, bpltv_duality_gap and the captured graphs stay untouched,
 * as with bpltv_vjp.  The residual gate, the image groups and the stats of the adjoint are bpltv_vjp's.  The active-set
 * weight is relative to the fidelity weight where that is small: an active element gets min(kappa, 4e14 * w_min), w_min the
 * smallest w of its nodes, so that no entry kappa s^2 of the scaled matrix passes 4e14 (nothing changes while w >= 1/4 at
 * kappa = 1e14; the result then moves by less than 1e-3 of 1e-8 max|p| from the system with kappa throughout, DESIGN.md
 * section 4.5); stats.kappa_used stays the kappa of the call. */
int bpltv_weighted_vjp(bpltv_t *h, const double *u, const double *f, const double *w, int wo, const double *alpha,
                       int am, int an, const bpltv_params *p, const double *gu,
                       double *grad_f_out, double *grad_alpha_out, double *grad_w_out);
/* The same with every array in HBM (device pointers); w, the parameter and the cotangent are checked on the device. */
int bpltv_weighted_vjp_device(bpltv_t *h, const double *d_u, const double *d_f, const double *d_w, int wo,
                              const double *d_alpha, int am, int an, const bpltv_params *p, const double *d_gu,
                              double *d_grad_f, double *d_grad_alpha, double *d_grad_w);

/* Reverse mode through the PDHG iterations themselves.  bpltv_vjp differentiates the exact minimiser
 * (the reference's adjoint system); these differentiate what a fixed number of iterations computed: the derivative of the
 * K-step map, exact for any K, with no active-set threshold, no kappa and no factorisation.  TV model, Float64 (also on
 * dtype = 32 handles), one parameter shared by the batch (alpha, am, an as bpltv_denoise); f is the resident dataset
 * (BPLTV_E_NODATA without one).
 *
 * bpltv_unrolled_denoise runs bpltv_denoise's recurrence with rho = 0, init = 0, order = 0 -- u is bpltv_denoise's bit for bit
 * -- and records, in every iteration, the dual before its projection: the tape, 2 * maxiter * M*N*O doubles
 * (bpltv_unrolled_tape_doubles; its layout is private).  params: opnorm, tau0, sigma0, accel, maxiter, tile_iters, use_graph,
 * reserved[1] and reserved[2] apply; rho, init and order must be 0 (BPLTV_E_UNSUPPORTED); check_every / gap_tol are ignored
 * (always maxiter iterations); maxiter < 1 is BPLTV_E_ARG.  The parameter is checked as bpltv_denoise checks it (finite and
 * >= 0, on the host or on the device); every rejection comes before anything of the handle changes.  The solve is a TV solve
 * and becomes the handle's last solve: bpltv_u_device, bpltv_copy_u_device and bpltv_duality_gap work as after bpltv_denoise.
 * stats: iterations, launches, tile_iters, tiles, pdhg_ms, total_ms; bytes_per_px_iter = 72 (scalar / patch parameter) or 80
 * (map); pdhg_variant = 0.  The results do not depend on tile_iters, on the launch chains or on use_graph, and the unrolled
 * calls never replay another solve's captured graphs, nor the reverse.
 *
 * The tape: d_tape is a caller-owned HBM buffer of bpltv_unrolled_tape_doubles doubles, so that two solves on one handle do not
 * overwrite each other's tape (the torch layer).  A NULL d_tape, and the host forms always, use a tape owned by the handle:
 * allocated on demand, only growing, freed by bpltv_destroy; when it cannot be allocated the call returns BPLTV_E_NOMEM and the
 * handle stays as it was.  The handle remembers maxiter, am, an and the step parameters (tau0, sigma0, accel, opnorm) its tape was
 * recorded with: a VJP on the handle's tape returns BPLTV_E_NODATA if there is none and BPLTV_E_ARG if they differ.  With a
 * caller's tape that match -- same handle geometry, same params, same parameter shape and VALUES as the solve that wrote it --
 * is the caller's contract; nothing checks it.
 *
 * bpltv_unrolled_vjp: for a cotangent gu = dL/du (M*N*O doubles, finite) grad_f_out = dL/df (M*N*O doubles) and grad_alpha_out
 * = dL/dalpha (am*an doubles: the per-pixel terms summed over the images in image order, then over all pixels, over each
 * patch, or not at all for a map; fixed order, no atomics).  Either output may be NULL, not both (BPLTV_E_ARG).  alpha must be the
 * parameter of the solve.  The VJP does not read f.  It stages its parameter apart, as bpltv_vjp does, and leaves the last
 * solve untouched.  stats: adjoint_ms is the HIP-event time of the reverse sweep, adjoint_method = 7.  Multi-device handles
 * over more than one shard: BPLTV_E_UNSUPPORTED (the four solve and VJP functions).
 *
 * Checkpointing: the tape grows with maxiter.  bpltv_set_option(h, "tape_checkpoint", C) with C != 0
 * trades it for one more forward solve, for this model, the weighted one and the sum of regularisers, shared and _each, host
 * and _device forms alike; C = 0 (the default) is everything described above, unchanged.  C >= 1 is the spacing in iterations,
 * Ceff = min(C, maxiter); C = -1 chooses Ceff = clamp(ceil(sqrt(nplanes * maxiter / tape_planes)), 1, maxiter), with nplanes /
 * tape_planes = 3 / 2 here, 3 / 3 weighted and 7 / 6 for the sum of regularisers: the spacing of least memory.
 *  - *_unrolled_tape_doubles returns nplanes * ceil(maxiter / Ceff) * M*N*O: one state set per segment of Ceff iterations, the
 *    state at its start (segment 0's too, so the count is never 0).  That is what a caller's d_tape must hold.
 *  - *_unrolled_denoise* runs the same recurrence -- u is still the plain denoise's bit for bit, and the solve becomes the
 *    handle's last solve as above -- with a kernel instantiation that stores no tape, and writes only those states, into
 *    d_tape or the handle's tape of the model.  stats.bytes_per_px_iter is the plain solve's (56 / 64 here, 64 / 72 weighted,
 *    120 / 144 sum of regularisers); the checkpoints are nplanes planes more per Ceff iterations, written in place of a state
 *    set by the launch that ends a segment.
 *  - *_unrolled_vjp* walks the segments from the last to the first: it re-runs a segment's iterations from its checkpoint with
 *    the taping kernel -- in state planes of its own, on the staged parameter (and weight) and the RESIDENT f, into a segment
 *    tape of tape_planes * Ceff * M*N*O doubles -- and reverses them with the reverse kernel, carrying its planes from segment
 *    to segment.  Same kernels, same state: every gradient is bitwise the full tape's.  The sweep therefore reads f for every
 *    model (BPLTV_E_NODATA without a dataset, before anything changes); d_tape stays const and is not written.  Segment tape
 *    and recompute planes belong to the handle: allocated on first use, only growing, freed by bpltv_destroy, BPLTV_E_NOMEM
 *    with the handle as it was when they cannot be had.  adjoint_ms includes the recompute; adjoint_method is unchanged.
 *  - The handle's tape remembers its spacing: a VJP on it under an option that gives another spacing (full against
 *    checkpointed included) is BPLTV_E_ARG.  bpltv_set_data(_device) invalidates a CHECKPOINTED handle tape -- its states no
 *    longer belong to the resident f -- and the next VJP on it is BPLTV_E_NODATA; a full tape is unaffected.  With a caller's
 *    buffer the spacing and the same resident f are part of the caller's contract.
 *  - As before the results do not depend on tile_iters, the launch chains, use_graph or whose buffer it is.  A call is one
 *    launch sequence (one graph per chain, all segments inside, keyed by the spacing), never one graph per segment. */
int bpltv_unrolled_tape_doubles(bpltv_t *h, const bpltv_params *p, unsigned long long *n_out);   /* 2*maxiter*M*N*O (option "tape_checkpoint" = 0) */
int bpltv_unrolled_denoise(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_unrolled_denoise_device(bpltv_t *h, const double *d_alpha, int am, int an, const bpltv_params *p, double *d_tape);
int bpltv_unrolled_vjp(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p,
                       const double *gu, double *grad_f_out, double *grad_alpha_out);
int bpltv_unrolled_vjp_device(bpltv_t *h, const double *d_tape, const double *d_alpha, int am, int an,
                              const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha);

/* Reverse mode through the PDHG iterations of the weighted model: what bpltv_unrolled_* is to
 * bpltv_denoise, for bpltv_weighted_denoise.  bpltv_weighted_vjp differentiates the exact minimiser and needs every w > 0;
 * these differentiate the K-step map itself, exactly for any K, with no factorisation, no kappa, no active-set threshold and
 * no w > 0: a mask (w in {0, 1}) gets gradients in f, alpha and w, and a learnable fidelity map gets dL/dw of the layer it is.
 * The contract is the union of the two existing ones.
 *
 * bpltv_weighted_unrolled_denoise: w, wo, alpha, am, an, params and every rejection as bpltv_weighted_denoise (w finite and
 * >= 0, wo = 1 or O, gamma = the smallest entry of ALL of w; rho, init and order must be 0, BPLTV_E_UNSUPPORTED; check_every /
 * gap_tol are ignored; Float64 on dtype = 32 handles too), and maxiter < 1 is BPLTV_E_ARG; reserved[1] and reserved[2] apply as
 * in bpltv_unrolled_denoise.  u is bpltv_weighted_denoise's bit for bit, for every w.  The solve becomes the handle's last
 * weighted solve: bpltv_u_device, bpltv_copy_u_device and bpltv_duality_gap behave as after bpltv_weighted_denoise.  In every
 * iteration it records the dual before its projection and the new primal iterate: the tape, 3 * maxiter * M*N*O doubles
 * (bpltv_weighted_unrolled_tape_doubles; its layout is private).  stats: as bpltv_weighted_denoise with bytes_per_px_iter = 88
 * (scalar / patch parameter) or 96 (map).
 *
 * The tape: d_tape is a caller-owned HBM buffer of bpltv_weighted_unrolled_tape_doubles doubles; a NULL d_tape, and the host
 * forms always, use a weighted tape owned by the handle (allocated on demand, only growing, freed by bpltv_destroy;
 * BPLTV_E_NOMEM, with the handle as it was, when it cannot be allocated).  It is not the tape of bpltv_unrolled_denoise: the
 * handle keeps the two apart, so a TV tape and a weighted tape are never accepted for each other's VJP, and either survives the
 * other model's solves.  The handle remembers maxiter, am, an, wo, gamma and the step parameters (tau0, sigma0, accel, opnorm)
 * its weighted tape was recorded with: a VJP on the handle's tape returns BPLTV_E_NODATA if there is none and BPLTV_E_ARG if
 * they differ.  With a caller's tape that match -- and the VALUES of w and alpha -- is the caller's contract.
 *
 * bpltv_weighted_unrolled_vjp: for a cotangent gu = dL/du (M*N*O doubles, finite) grad_f_out = dL/df (M*N*O doubles),
 * grad_alpha_out = dL/dalpha (am*an doubles, reduced as bpltv_unrolled_vjp reduces it) and grad_w_out = dL/dw (M*N*wo doubles;
 * for wo = 1 the sum over the images in image order); fixed order, no atomics.  Any output may be NULL, not all three
 * (BPLTV_E_ARG).  w and alpha must be those of the solve; w is checked as the solve checks it (>= 0, zeros are legal).  At
 * w = 0, grad_w is the one-sided derivative.  The resident f is read for grad_w only (BPLTV_E_NODATA without a dataset when
 * grad_w_out is given).  The step table depends on gamma = min w; the VJP holds it fixed: exact for accel = 0 and for
 * gamma = 0 (every mask), while with gamma > 0 and acceleration the derivative through the step sizes -- which touches only
 * the entries of w that attain the minimum -- is omitted.  With w == 1, grad_f and grad_alpha agree with bpltv_unrolled_vjp's
 * to rounding (u bit for bit).  Every rejection comes before anything of the handle changes; w and the parameter are staged
 * apart and the last solve stays untouched.  stats: only adjoint_ms (the HIP-event time of the reverse sweep) and
 * adjoint_method = 9 change.  The results do not depend on tile_iters, on the launch chains, on use_graph, on the host or
 * device form or on whose tape it is, and these calls never replay the captured graphs of the TV, sum-of-regularisers,
 * weighted or unrolled calls, nor the reverse.  Multi-device handles over more than one shard: BPLTV_E_UNSUPPORTED (all five);
 * one shard is forwarded. */
int bpltv_weighted_unrolled_tape_doubles(bpltv_t *h, const bpltv_params *p, unsigned long long *n_out);   /* 3*maxiter*M*N*O; option "tape_checkpoint": see bpltv_unrolled_tape_doubles */
int bpltv_weighted_unrolled_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                    const bpltv_params *p, double *u_out);
int bpltv_weighted_unrolled_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                           const bpltv_params *p, double *d_tape);
int bpltv_weighted_unrolled_vjp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                const bpltv_params *p, const double *gu,
                                double *grad_f_out, double *grad_alpha_out, double *grad_w_out);
int bpltv_weighted_unrolled_vjp_device(bpltv_t *h, const double *d_tape, const double *d_w, int wo, const double *d_alpha,
                                       int am, int an, const bpltv_params *p, const double *d_gu,
                                       double *d_grad_f, double *d_grad_alpha, double *d_grad_w);

/* Forward mode through the PDHG iterations: the tangent of the K-step map that bpltv_unrolled_vjp
 * transposes -- <gu, du> = <grad_f(gu), df> + <grad_alpha(gu), dalpha> for any gu -- exact for any K, with no tape: a sweep
 * carries (dx, dy1, dy2) beside (x, y1, y2) in 14 planes of M*N*O doubles owned by the handle (allocated on first use, freed by
 * bpltv_destroy; BPLTV_E_NOMEM, with the handle as it was, when they cannot be allocated), whatever maxiter is.  TV model,
 * Float64 (also on dtype = 32 handles), one parameter shared by the batch; f is the resident dataset (BPLTV_E_NODATA without
 * one).  params as for bpltv_unrolled_denoise: rho, init and order must be 0 (BPLTV_E_UNSUPPORTED), maxiter < 1 is BPLTV_E_ARG,
 * check_every / gap_tol are ignored.
 *
 * bpltv_unrolled_jvp: ndir >= 1 directions, direction-major: df is NULL or ndir * M*N*O doubles, dalpha NULL or ndir * am*an
 * doubles indexed as alpha is, not both NULL (a NULL tangent is zero); du_out: ndir * M*N*O doubles.  The directions are swept
 * one after the other: direction d of a call is bitwise the ndir = 1 call with that direction.  u_out (may be NULL): the primal
 * result, M*N*O doubles, bpltv_denoise's u bit for bit.  alpha is checked as bpltv_denoise checks it (finite, >= 0) and the
 * tangents must be finite (the host form checks them on the host, the device form on the device); ndir < 1, both tangents
 * NULL, a bad parameter shape or a NULL du_out is BPLTV_E_ARG; every rejection comes before anything of the handle changes.
 * The sweep stages its parameter and its tangents apart and runs in planes of its own: the last solve, bpltv_u_device,
 * bpltv_duality_gap, the handle's tape and the solve statistics stay as they were, and it never replays a taped solve's or a
 * reverse sweep's captured graphs, nor they its.  stats: only adjoint_ms (the HIP-event time of the sweeps) and adjoint_method
 * = 8 change.  The results do not depend on tile_iters, on the launch chains or on use_graph.
 *
 * bpltv_unrolled_gauss_newton: for a scalar or a patch parameter of P = am*an <= 16 entries (anything else:
 * BPLTV_E_UNSUPPORTED), P unit-direction sweeps (columns in the parameter's column-major order) and, with ubar the resident
 * dataset's, cost_out = 0.5||u_K - ubar||^2, grad_out = J^T (u_K - ubar) (P doubles) and hess_out = J^T J (P x P, column major,
 * symmetric bit for bit) of the K-step loss; sums per image, then over the images in image order.
 * Multi-device handles over more than one shard: BPLTV_E_UNSUPPORTED (all three). */
int bpltv_unrolled_jvp(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p, int ndir,
                       const double *df, const double *dalpha, double *du_out, double *u_out /* may be NULL */);
int bpltv_unrolled_jvp_device(bpltv_t *h, const double *d_alpha, int am, int an, const bpltv_params *p, int ndir,
                              const double *d_df, const double *d_dalpha, double *d_du, double *d_u /* may be NULL */);
int bpltv_unrolled_gauss_newton(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p,
                                double *cost_out, double *grad_out, double *hess_out);

/* Forward mode through the PDHG iterations of the weighted model: the tangent of the K-step map that
 * bpltv_weighted_unrolled_vjp transposes -- <gu, du> = <grad_f(gu), df> + <grad_alpha(gu), dalpha> + <grad_w(gu), dw> for any
 * gu -- with no tape and, like that VJP, no w > 0: a mask (w in {0, 1}) has sensitivities in f, alpha and w.  A sweep carries
 * (dx, dy1, dy2) beside (x, y1, y2) in 16 planes of M*N*O doubles (two state sets of six planes, then the staged df, dalpha, w
 * and dw) and 8 check words, owned by the handle and apart from the TV sweep's 14 (allocated on first use, freed by
 * bpltv_destroy; BPLTV_E_NOMEM, with the handle as it was, when they cannot be allocated), whatever maxiter is.  Float64 (also
 * on dtype = 32 handles), one parameter shared by the batch; f is the resident dataset (BPLTV_E_NODATA without one).  The
 * contract is the union of bpltv_unrolled_jvp's and bpltv_weighted_unrolled_denoise's.
 *
 * bpltv_weighted_unrolled_jvp: w, wo, alpha, am, an and params as bpltv_weighted_unrolled_denoise (w and alpha finite and >= 0,
 * zeros legal, wo = 1 or O; rho, init and order must be 0, BPLTV_E_UNSUPPORTED; maxiter < 1 is BPLTV_E_ARG; check_every, gap_tol
 * and the option "tape_checkpoint" are ignored).  ndir >= 1 directions, direction-major: df is NULL or ndir * M*N*O doubles,
 * dalpha NULL or ndir * am*an doubles indexed as alpha is, dw NULL or ndir * M*N*wo doubles laid out as w is (wo = 1: one plane
 * shared by all images), not all three NULL (a NULL tangent is zero and is not loaded); du_out: ndir * M*N*O doubles.  Direction
 * d of a call is bitwise the ndir = 1 call with that direction.  u_out (may be NULL): the primal result, M*N*O doubles,
 * bpltv_weighted_denoise's u bit for bit.  The tangents must be finite (the host form checks them on the host, the device form
 * on the device); ndir < 1, all tangents NULL, a bad wo or parameter shape or a NULL du_out is BPLTV_E_ARG; every rejection
 * comes before anything of the handle changes.  At w = 0, dw is the one-sided derivative.  The step table depends on gamma =
 * min w; the sweep holds it fixed, exactly as bpltv_weighted_unrolled_vjp does, so it is that VJP's exact transpose: exact for
 * accel = 0 and for gamma = 0 (every mask), while with gamma > 0 and acceleration the derivative through the step sizes --
 * which touches only the entries of w that attain the minimum -- is omitted.  With w == 1 and dw NULL, du agrees with
 * bpltv_unrolled_jvp's to rounding (u bit for bit).  The sweep stages w, the parameter and the tangents apart and runs in planes
 * of its own: the last solve, bpltv_u_device, bpltv_duality_gap, the three tapes and the solve statistics stay as they were,
 * and it shares no captured graph with any other call.  stats: only adjoint_ms (the HIP-event time of the sweeps) and
 * adjoint_method = 11 change.  The results do not depend on tile_iters, on the launch chains, on use_graph or on the host or
 * device form.
 *
 * bpltv_weighted_unrolled_gauss_newton: as bpltv_unrolled_gauss_newton, for the weighted iterations: a scalar or a patch
 * parameter of P = am*an <= 16 entries (anything else: BPLTV_E_UNSUPPORTED), P unit-direction sweeps in alpha and, with ubar the
 * resident dataset's, cost_out = 0.5||u_K - ubar||^2, grad_out = J^T (u_K - ubar) and hess_out = J^T J (P x P, column major,
 * symmetric bit for bit); sums per image, then over the images in image order, no atomics.
 * Multi-device handles over more than one shard: BPLTV_E_UNSUPPORTED (all three); one shard is forwarded. */
int bpltv_weighted_unrolled_jvp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                const bpltv_params *p, int ndir, const double *df, const double *dalpha, const double *dw,
                                double *du_out, double *u_out /* may be NULL */);
int bpltv_weighted_unrolled_jvp_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                       const bpltv_params *p, int ndir, const double *d_df, const double *d_dalpha,
                                       const double *d_dw, double *d_du, double *d_u /* may be NULL */);
int bpltv_weighted_unrolled_gauss_newton(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                         const bpltv_params *p, double *cost_out, double *grad_out, double *hess_out);

/* The unrolled solve, VJP and JVP with one parameter per image: what a network that predicts alpha per sample needs at a
 * small, fixed iteration count.  alphas: O blocks of am x an doubles, column major, block k at alphas + k*am*an, image k
 * reads block k (bpltv_denoise_each's layout, bpltv_denoise's shape rules).  Each function keeps the contract of its shared
 * twin above -- params, rejections and their codes, what becomes or stays the last solve, the tapes, the statistics
 * (bytes_per_px_iter 72 / 80, adjoint_method 7 / 8), independence of tile_iters, launch chains and use_graph, dtype = 32
 * handles in Float64, multi-device handles forwarded on one shard and BPLTV_E_UNSUPPORTED beyond -- with these differences:
 *  - every entry of every block is checked (finite, >= 0; 0 is legal), on the host or on the device, before anything of the
 *    handle changes;
 *  - u of image k is bitwise the one-image solve with block k, the whole u bitwise bpltv_denoise_each's, and after
 *    bpltv_unrolled_denoise_each bpltv_duality_gap evaluates image k with its own block;
 *  - the tape has the shared size and layout (bpltv_unrolled_tape_doubles).  The handle's tape remembers whether it was
 *    recorded per image: bpltv_unrolled_vjp on a per-image tape and bpltv_unrolled_vjp_each on a shared one return
 *    BPLTV_E_ARG.  A caller's tape stays the caller's contract;
 *  - grad_alphas_out: O blocks of am*an doubles, block k being image k's term alone (the per-pixel plane as it is for a map,
 *    image k's sums over all pixels or over each patch otherwise; fixed order, no atomics).  With equal blocks, the blocks
 *    added in image order are bpltv_unrolled_vjp's grad_alpha_out bit for bit;
 *  - dalphas: NULL or ndir x O blocks of am*an doubles, direction first, then image (bpltv_jvp_each's layout); image k's du
 *    is bitwise the one-image sweep with (df_k, dalpha_k);
 *  - a per-image call never replays a shared call's captured graph, nor the reverse. */
int bpltv_unrolled_denoise_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_unrolled_denoise_each_device(bpltv_t *h, const double *d_alphas, int am, int an, const bpltv_params *p, double *d_tape);
int bpltv_unrolled_vjp_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p,
                            const double *gu, double *grad_f_out, double *grad_alphas_out);
int bpltv_unrolled_vjp_each_device(bpltv_t *h, const double *d_tape, const double *d_alphas, int am, int an,
                                   const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alphas);
int bpltv_unrolled_jvp_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p, int ndir,
                            const double *df, const double *dalphas, double *du_out, double *u_out /* may be NULL */);
int bpltv_unrolled_jvp_each_device(bpltv_t *h, const double *d_alphas, int am, int an, const bpltv_params *p, int ndir,
                                   const double *d_df, const double *d_dalphas, double *d_du, double *d_u /* may be NULL */);

/* Reverse mode through the PDHG iterations of the sum-of-regularisers model: what bpltv_unrolled_* is
 * to bpltv_denoise, for bpltv_sumregs_denoise -- the exact derivative of the maxiter-step map, with no active-set threshold, no
 * factorisation and no condition on the parameter beyond >= 0, where bpltv_sumregs_vjp differentiates the minimiser.
 *
 * bpltv_sumregs_unrolled_denoise: alpha, am, an as bpltv_sumregs_denoise (3*am*an doubles, the three slices one after the
 * other; finite and >= 0, checked on the host or on the device; zeros are legal, a whole slice of zeros included), BPLTV_E_NODATA
 * without a dataset.  params (NULL: bpltv_sumregs_default_params): opnorm, tau0, sigma0, accel, maxiter, tile_iters, use_graph,
 * reserved[1] and reserved[2] apply; rho, init and order must be 0 (BPLTV_E_UNSUPPORTED), maxiter < 1 is BPLTV_E_ARG,
 * check_every and gap_tol are ignored (always maxiter iterations), and reserved[0], the forward variant, is ignored: there is
 * one taped kernel.  u is bpltv_sumregs_denoise's bit for bit, for either of its variants.  The solve is a sum-of-regularisers
 * solve and becomes the handle's last one: bpltv_u_device, bpltv_copy_u_device and bpltv_duality_gap behave as after
 * bpltv_sumregs_denoise.  It also records the six dual components before their projection in every iteration: a tape of
 * 6 * maxiter * M*N*O doubles (bpltv_sumregs_unrolled_tape_doubles; its layout is private).  stats: iterations, launches,
 * tile_iters, tiles, pdhg_ms, total_ms as bpltv_sumregs_denoise; bytes_per_px_iter = 168 (192 with three maps);
 * pdhg_variant = 0.  Every rejection comes before anything of the handle changes.
 *
 * The tape: d_tape is a caller-owned HBM buffer of bpltv_sumregs_unrolled_tape_doubles doubles; a NULL d_tape, and the host
 * forms always, use a tape owned by the handle (allocated on demand, only grows, freed by bpltv_destroy; BPLTV_E_NOMEM, with the
 * handle as it was, when it cannot be allocated).  It is a third tape beside those of bpltv_unrolled_denoise and
 * bpltv_weighted_unrolled_denoise: none is accepted for another model's VJP and each survives the other models' solves.  The
 * handle remembers maxiter, am, an, the step parameters and whether the tape was recorded per image; a VJP on the handle's tape
 * returns BPLTV_E_NODATA when there is none and BPLTV_E_ARG on any mismatch (the shared form on a per-image tape, and the
 * reverse, included).
 *
 * bpltv_sumregs_unrolled_vjp: for a cotangent gu = dL/du (M*N*O doubles, finite) grad_f_out = dL/df (M*N*O doubles) and
 * grad_alpha_out = dL/dalpha (3*am*an doubles; every slice reduced as bpltv_unrolled_vjp reduces its parameter: over the images
 * in image order, then over all pixels, each patch, or nothing for a map -- fixed order, no atomics).  Either output may be
 * NULL, not both.  alpha and params must be the solve's.  f is not read.  The parameter is staged apart and the last solve
 * stays untouched; of the statistics only adjoint_ms (the HIP-event time of the sweep) and adjoint_method = 10 change.  The
 * results do not depend on tile_iters, on the launch chains, on use_graph, on the host or device form, or on whose tape it is.
 *
 * The _each forms take one block of 3*am*an doubles per image (bpltv_sumregs_denoise_each's layout) and have the contract of
 * their shared twins; after the solve bpltv_duality_gap evaluates image k with its own block.  grad_alphas_out: O blocks, block
 * k image k's own.  Image k's results are bitwise the one-image handle's with block k; with equal blocks, the blocks added in
 * image order are the shared form's grad_alpha_out bit for bit, and grad_f is equal bitwise.
 *
 * No captured graph is shared with bpltv_sumregs_denoise, the TV, weighted or other unrolled calls.  Multi-device handles over
 * more than one shard: BPLTV_E_UNSUPPORTED (all nine); one shard is forwarded.  dtype = 32 handles behave as
 * bpltv_sumregs_denoise does on them; these calls always compute in Float64. */
int bpltv_sumregs_unrolled_tape_doubles(bpltv_t *h, const bpltv_params *p, unsigned long long *n_out);   /* 6*maxiter*M*N*O; option "tape_checkpoint": see bpltv_unrolled_tape_doubles */
int bpltv_sumregs_unrolled_denoise(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_sumregs_unrolled_denoise_device(bpltv_t *h, const double *d_alpha, int am, int an, const bpltv_params *p, double *d_tape);
int bpltv_sumregs_unrolled_vjp(bpltv_t *h, const double *alpha, int am, int an, const bpltv_params *p,
                               const double *gu, double *grad_f_out, double *grad_alpha_out);
int bpltv_sumregs_unrolled_vjp_device(bpltv_t *h, const double *d_tape, const double *d_alpha, int am, int an,
                                      const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha);
int bpltv_sumregs_unrolled_denoise_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_sumregs_unrolled_denoise_each_device(bpltv_t *h, const double *d_alphas, int am, int an, const bpltv_params *p,
                                               double *d_tape);
int bpltv_sumregs_unrolled_vjp_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p,
                                    const double *gu, double *grad_f_out, double *grad_alphas_out);
int bpltv_sumregs_unrolled_vjp_each_device(bpltv_t *h, const double *d_tape, const double *d_alphas, int am, int an,
                                           const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alphas);

/* Channel-coupled (vectorial) TV for colour images:
 *
 *     min_u  1/2 sum_c |u_c - f_c|^2  +  sum_pixels alpha * sqrt( sum_c |(grad u_c)|^2 )
 *
 * The handle's O planes are O / channels colour images: image b owns the planes b*channels ... b*channels + channels-1 (a
 * contiguous (B, C, H, W) array as it is).  alpha is one parameter shared by the batch and by the channels: scalar, patch or
 * per-pixel map, with bpltv_denoise's shape rules and upsampling.  The iteration is bpltv_unrolled_denoise's per plane; only
 * the projection couples the channels: every pixel of a colour image projects the 2*channels dual values of its planes onto
 * one ball of radius alpha.  channels = 1 returns the bits of the bpltv_unrolled_* calls.
 *
 * The contract is bpltv_unrolled_denoise's and bpltv_unrolled_vjp's: params opnorm, tau0, sigma0, accel, maxiter, tile_iters,
 * use_graph, reserved[1] and reserved[2] apply; rho, init and order must be 0 (BPLTV_E_UNSUPPORTED), maxiter < 1 is
 * BPLTV_E_ARG, check_every and gap_tol are ignored; alpha is checked finite and >= 0 on the host or on the device; every
 * rejection comes before anything of the handle changes.  In addition channels outside 1 ... 4, or not dividing O, is
 * BPLTV_E_ARG.  The results do not depend on tile_iters, on the launch chains (a chain never splits a colour image), on
 * use_graph, on the host or device form, or on whose tape it is.  dtype = 32 handles compute in Float64.  Multi-device handles
 * over more than one shard: BPLTV_E_UNSUPPORTED; one shard is forwarded.
 *
 * bpltv_color_denoise: the recurrence without a tape, for any maxiter >= 1; u is bitwise the taped solve's.  It touches no tape.
 * bpltv_color_unrolled_denoise: the same and the tape of the dual values before the projection, in the TV tape's layout and
 * size: bpltv_unrolled_tape_doubles gives the doubles of a caller-owned d_tape (option "tape_checkpoint" included).  A NULL
 * d_tape, and the host form always, use a fourth tape owned by the handle, which remembers channels.  It is never accepted by
 * bpltv_unrolled_vjp, nor a TV tape by bpltv_color_unrolled_vjp, and each survives the other models' solves.
 * Either solve becomes the handle's last one for bpltv_u_device / bpltv_copy_u_device.  bpltv_duality_gap after it returns
 * BPLTV_E_UNSUPPORTED, until another model solves: the gap of the coupled model is not implemented.  stats: as
 * bpltv_unrolled_denoise, with tiles counting workgroups (tiles times colour images) and bytes_per_px_iter per plane: 72
 * (56 without a tape), plus 8 / channels with a map, which the planes of a colour image share; pdhg_variant = 0.
 *
 * bpltv_color_unrolled_vjp: the exact reverse mode through the iterations, as bpltv_unrolled_vjp: gu and grad_f_out have M*N*O
 * doubles, grad_alpha_out am*an (summed over the colour images in image order, then as bpltv_unrolled_vjp reduces).  channels,
 * alpha and params must be the solve's: BPLTV_E_ARG on the handle's tape otherwise.  Of the statistics only adjoint_ms and
 * adjoint_method = 12 change. */
int bpltv_color_denoise(bpltv_t *h, int channels, const double *alpha, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_color_denoise_device(bpltv_t *h, int channels, const double *d_alpha, int am, int an, const bpltv_params *p);
int bpltv_color_unrolled_denoise(bpltv_t *h, int channels, const double *alpha, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_color_unrolled_denoise_device(bpltv_t *h, int channels, const double *d_alpha, int am, int an, const bpltv_params *p, double *d_tape);
int bpltv_color_unrolled_vjp(bpltv_t *h, int channels, const double *alpha, int am, int an, const bpltv_params *p,
                             const double *gu, double *grad_f_out, double *grad_alpha_out);
int bpltv_color_unrolled_vjp_device(bpltv_t *h, int channels, const double *d_tape, const double *d_alpha, int am, int an,
                                    const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha);

/* Channel-coupled TV with a per-pixel data-fidelity weight: colour inpainting (one mask for the
 * channels), demosaicing (a mask per channel), a noise variance per channel, a learned fidelity map.
 *
 *     min_u  1/2 sum_c sum_pixels w_c (u_c - f_c)^2  +  sum_pixels alpha * sqrt( sum_c |(grad u_c)|^2 ),      w >= 0
 *
 * Planes and alpha as bpltv_color_denoise; w as bpltv_weighted_denoise: wo = 1 (one plane for all O planes) or wo = O (one per
 * plane, that is per channel of every colour image); a caller with one mask per colour image passes it expanded to O planes.
 * gamma = min w over everything passed goes into the step table (a mask: gamma = 0, omega = 1, and accel changes nothing).  The
 * primal step of every plane is bpltv_weighted_unrolled_denoise's, the projection bpltv_color_denoise's.  channels = 1 returns
 * the bits of the bpltv_weighted_unrolled_* calls; w == 1 the bits of bpltv_color_denoise.
 *
 * The contract is the union of bpltv_color_unrolled_*'s and bpltv_weighted_unrolled_*'s: channels outside 1 ... 4 or not
 * dividing O, wo other than 1 or O, a NULL, negative or non-finite w, maxiter < 1 and a bad parameter are BPLTV_E_ARG; rho, init
 * and order must be 0 (BPLTV_E_UNSUPPORTED); no data is BPLTV_E_NODATA; multi-device handles over more than one shard are
 * BPLTV_E_UNSUPPORTED; every rejection comes before anything of the handle changes.  The results do not depend on tile_iters, on
 * the launch chains, on use_graph, on the host or device form, on whose tape it is, or on option "tape_checkpoint".
 *
 * bpltv_color_weighted_denoise: the recurrence without a tape; u is bitwise the taped solve's.
 * bpltv_color_weighted_unrolled_denoise: the same and the tape of z1, z2 (before the projection) and x+ of every plane, in the
 * weighted tape's layout and size: bpltv_weighted_unrolled_tape_doubles gives the doubles of a caller-owned d_tape.  A NULL
 * d_tape, and the host form always, use a fifth tape owned by the handle, which remembers channels, wo and gamma.  No other
 * model's sweep accepts it, nor this sweep a TV, weighted or colour tape, and each survives the others' solves.  Either solve
 * becomes the handle's last one for bpltv_u_device / bpltv_copy_u_device; bpltv_duality_gap after it is BPLTV_E_UNSUPPORTED.
 * stats: as bpltv_color_unrolled_denoise, with bytes_per_px_iter 88 (64 without a tape) per plane, plus 8 / channels with a map.
 *
 * bpltv_color_weighted_unrolled_vjp: the exact reverse mode through the iterations with the step table held fixed (exact for
 * masks and for accel = 0): grad_f_out M*N*O doubles, grad_alpha_out am*an, grad_w_out w's shape (wo = 1: summed over the planes
 * in plane order); any may be NULL, not all three.  channels, w's planes and gamma, alpha's shape and params must be the
 * solve's: BPLTV_E_ARG on the handle's tape otherwise; no colour-weighted tape, or grad_w_out without a dataset, is
 * BPLTV_E_NODATA.  Of the statistics only adjoint_ms and adjoint_method = 14 change. */
int bpltv_color_weighted_denoise(bpltv_t *h, int channels, const double *w, int wo, const double *alpha, int am, int an,
                                 const bpltv_params *p, double *u_out);
int bpltv_color_weighted_denoise_device(bpltv_t *h, int channels, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                        const bpltv_params *p);
int bpltv_color_weighted_unrolled_denoise(bpltv_t *h, int channels, const double *w, int wo, const double *alpha, int am, int an,
                                          const bpltv_params *p, double *u_out);
int bpltv_color_weighted_unrolled_denoise_device(bpltv_t *h, int channels, const double *d_w, int wo, const double *d_alpha, int am,
                                                 int an, const bpltv_params *p, double *d_tape);
int bpltv_color_weighted_unrolled_vjp(bpltv_t *h, int channels, const double *w, int wo, const double *alpha, int am, int an,
                                      const bpltv_params *p, const double *gu, double *grad_f_out, double *grad_alpha_out,
                                      double *grad_w_out);
int bpltv_color_weighted_unrolled_vjp_device(bpltv_t *h, int channels, const double *d_tape, const double *d_w, int wo,
                                             const double *d_alpha, int am, int an, const bpltv_params *p, const double *d_gu,
                                             double *d_grad_f, double *d_grad_alpha, double *d_grad_w);

/* TV-L1 denoising: the absolute value in place of the square in the data term -- the model for
 * salt-and-pepper noise, outliers and dead pixels, which a quadratic term smears into blobs ("lone": L-one; the names of this
 * interface hold no digits):
 *
 *     min_u  sum_pixels w |u - f|  +  sum_pixels alpha |grad u|,      w >= 0
 *
 * Grey planes, Float64.  alpha as bpltv_denoise (scalar, patch or map); w as bpltv_weighted_denoise: wo = 1 (one plane for all O
 * images) or wo = O, zeros legal (a pixel without data).  The data term has no strong convexity, so the step table is made with
 * gamma = 0 whatever w is: omega = 1, constant steps, and accel = 0 and 1 give the same bits.  Iteration k, from x = f, y = 0, is
 * bpltv_weighted_unrolled_denoise's except for the primal step, a soft threshold around f (explicit fma, no division):
 *
 *     v = fma(-tau_k, G^T y, x);  d = v - f;  m = |d| - tau_k*w;  x+ = m > 0 ? f + copysign(m, d) : f
 *
 * The contract is bpltv_weighted_unrolled_*'s: wo other than 1 or O, a NULL, negative or non-finite w, maxiter < 1 and a bad
 * parameter are BPLTV_E_ARG; rho, init and order must be 0 (BPLTV_E_UNSUPPORTED); no data is BPLTV_E_NODATA; check_every and
 * gap_tol are ignored; dtype = 32 handles compute in Float64; a multi-device handle forwards to its one shard and is
 * BPLTV_E_UNSUPPORTED over more; every rejection comes before anything of the handle changes.  The results do not depend on
 * tile_iters, on the launch chains, on use_graph, on the host or device form, on whose tape it is, or on option
 * "tape_checkpoint".
 *
 * bpltv_lone_denoise: the recurrence without a tape; u is bitwise the taped solve's.
 * bpltv_lone_unrolled_denoise: the same and the tape of z1, z2 (before the projection) and x+, in the weighted tape's layout and
 * size: bpltv_weighted_unrolled_tape_doubles gives the doubles of a caller-owned d_tape.  A NULL d_tape, and the host form
 * always, use a sixth tape owned by the handle, which remembers wo.  No other model's sweep accepts it, nor this sweep another
 * model's tape, and each survives the others' solves; no captured graph is shared with the weighted model.  Either solve becomes
 * the handle's last one for bpltv_u_device / bpltv_copy_u_device; bpltv_duality_gap after it is BPLTV_E_UNSUPPORTED until
 * another model solves (the L1 dual has a pointwise constraint the iterate does not meet).
 * stats: as bpltv_weighted_unrolled_denoise.  bytes_per_px_iter, from what the kernels load and store per pixel and iteration of
 * a launch of one iteration: read x, y1, y2, f, w (40 bytes; + 8 for alpha with a map), write x, y1, y2 (24) -- 64 / 72 without a
 * tape -- and write z1, z2, x+ onto the tape (24): 88 / 96.
 *
 * bpltv_lone_unrolled_vjp: reverse mode through the iterations, exact wherever no pixel sits on the threshold (the step table does
 * not depend on w or alpha).  The tail of reverse step k decides on the tape alone:
 *
 *     act = (x+ != f) || (w == 0);  h = act ? gxn : 0;  gf += act ? 0 : gxn;  gw += -tau_k * (sign(x+ - f) * h)
 *     gy = gz - tau_k * G h;  gx = h - omega_k * gxb
 *
 * (w == 0: the threshold is the identity, whatever d is, and so is its derivative; grad_w there is the one-sided derivative
 * -tau_k * sign(d) * h, which is a choice of subgradient where d is zero up to rounding.)
 * grad_f_out M*N*O doubles, grad_alpha_out am*an, grad_w_out w's shape (wo = 1: summed over the images in image order); any may
 * be NULL, not all three.  The sweep always reads the resident f.  w's planes, alpha's shape and params must be the solve's:
 * BPLTV_E_ARG on the handle's tape otherwise; no L1 tape or no dataset is BPLTV_E_NODATA.  Of the statistics only adjoint_ms
 * and adjoint_method = 15 change. */
int bpltv_lone_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                     double *u_out);
int bpltv_lone_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an, const bpltv_params *p);
int bpltv_lone_unrolled_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                              double *u_out);
int bpltv_lone_unrolled_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                     const bpltv_params *p, double *d_tape);
int bpltv_lone_unrolled_vjp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                          const double *gu, double *grad_f_out, double *grad_alpha_out, double *grad_w_out);
int bpltv_lone_unrolled_vjp_device(bpltv_t *h, const double *d_tape, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                 const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha, double *d_grad_w);

/* TV-KL denoising: the Kullback-Leibler divergence as the data term -- the model for Poisson noise
 * (photon counts: microscopy, astronomy, low-dose imaging), whose variance grows with the signal, so that a quadratic term
 * over-smooths the dark regions and under-smooths the bright ones:
 *
 *     min_u  sum_pixels w (u - f log u)  +  sum_pixels alpha |grad u|,      w >= 0,  f >= 0,  u >= 0
 *
 * Grey planes, Float64.  alpha as bpltv_denoise (scalar, patch or map); w as bpltv_weighted_denoise: wo = 1 (one plane for all O
 * images) or wo = O, zeros legal (a pixel without data).  f is the handle's dataset and must be finite and >= 0; zero counts are
 * legal.  The data term is strongly convex on bounded sets only, so the step table is made with gamma = 0 whatever w is:
 * omega = 1, constant steps, and accel = 0 and 1 give the same bits.  Iteration k, from x = f, y = 0, is
 * bpltv_weighted_unrolled_denoise's except for the primal step, the prox of the data term in closed form (explicit fma; IEEE
 * square root and division):
 *
 *     v = fma(-tau_k, G^T y, x);  t = tau_k*w;  c = v - t;  g = t*f;  s = sqrt(c*c + 4*g)
 *     x+ = (c >= 0) ? 0.5*(c + s) : (2*g) / (s - c)
 *
 * Both branches are the positive root of u^2 - c u - t f = 0; the second has no cancellation when t is large (w = 1e30 returns f
 * to rounding), and c < 0 gives s - c > 0.  w = 0 or f = 0 gives x+ = max(c, 0): a pixel without data is inpainted under u >= 0.
 *
 * The contract is bpltv_weighted_unrolled_*'s: wo other than 1 or O, a NULL, negative or non-finite w, maxiter < 1 and a bad
 * parameter are BPLTV_E_ARG; rho, init and order must be 0 (BPLTV_E_UNSUPPORTED); no data is BPLTV_E_NODATA; check_every and
 * gap_tol are ignored; dtype = 32 handles compute in Float64; a multi-device handle forwards to its one shard and is
 * BPLTV_E_UNSUPPORTED over more.  One rule more: a dataset with a negative or non-finite entry is BPLTV_E_ARG for the three
 * solves, with a message that names f; the dataset is looked at once after each bpltv_set_data(_device) and the answer kept,
 * and the other models take the same dataset as before.  Every rejection comes before anything of the handle changes.  The
 * results do not depend on tile_iters, on the launch chains, on use_graph, on the host or device form, on whose tape it is, or on
 * option "tape_checkpoint".
 *
 * bpltv_kl_denoise: the recurrence without a tape; u is bitwise the taped solve's.
 * bpltv_kl_unrolled_denoise: the same and the tape of z1, z2 (before the projection) and x+, in the weighted tape's layout and
 * size: bpltv_weighted_unrolled_tape_doubles gives the doubles of a caller-owned d_tape.  A NULL d_tape, and the host form
 * always, use a seventh tape owned by the handle, which remembers wo.  No other model's sweep accepts it, nor this sweep another
 * model's tape, and each survives the others' solves; no captured graph is shared with the weighted or the TV-L1 model.  Either
 * solve becomes the handle's last one for bpltv_u_device / bpltv_copy_u_device; bpltv_duality_gap after it is
 * BPLTV_E_UNSUPPORTED until another model solves (the gap of this data term is not implemented).
 * stats: as bpltv_weighted_unrolled_denoise.  bytes_per_px_iter, from what the kernels load and store per pixel and iteration of
 * a launch of one iteration: read x, y1, y2, f, w (40 bytes; + 8 for alpha with a map), write x, y1, y2 (24) -- 64 / 72 without a
 * tape -- and write z1, z2, x+ onto the tape (24): 88 / 96.
 *
 * bpltv_kl_unrolled_vjp: reverse mode through the iterations.  The step table depends on neither w nor alpha, and the primal
 * step has no kink where w f > 0, so the derivative is exact wherever x+ > 0.  The tail of reverse step k needs only the tape, f,
 * w and tau_k:
 *
 *     t = tau_k*w;  D = fma(t, f, x+*x+);  q = (D > 0) ? x+ / D : 0;  e = q*gxn          (e = gxn / s, since s = x+ + t f / x+)
 *     h = x+*e;  gf += t*e;  gw += tau_k*((f - x+)*e);  gy = gz - tau_k * G h;  gx = h - omega_k * gxb
 *
 * (dx+/dv = x+/s, dx+/df = tau w/s, dx+/dw = tau (f - x+)/s.)  Convention: where x+ = 0 exactly -- possible only where w f = 0 and
 * the iterate was clamped at zero -- the tail passes nothing (q = 0); the one-sided terms tau w/|c| of grad_f and tau f/|c| of
 * grad_w there, which the tape cannot give, are dropped.
 * grad_f_out M*N*O doubles, grad_alpha_out am*an, grad_w_out w's shape (wo = 1: summed over the images in image order); any may
 * be NULL, not all three.  The sweep always reads the resident f (and does not look at its sign).  w's planes, alpha's shape and
 * params must be the solve's: BPLTV_E_ARG on the handle's tape otherwise; no KL tape or no dataset is BPLTV_E_NODATA.  Of the
 * statistics only adjoint_ms and adjoint_method = 16 change. */
int bpltv_kl_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                     double *u_out);
int bpltv_kl_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an, const bpltv_params *p);
int bpltv_kl_unrolled_denoise(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                              double *u_out);
int bpltv_kl_unrolled_denoise_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                     const bpltv_params *p, double *d_tape);
int bpltv_kl_unrolled_vjp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an, const bpltv_params *p,
                          const double *gu, double *grad_f_out, double *grad_alpha_out, double *grad_w_out);
int bpltv_kl_unrolled_vjp_device(bpltv_t *h, const double *d_tape, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                 const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha, double *d_grad_w);

/* Forward mode through the TV-L1 and the TV-KL iterations: bpltv_weighted_unrolled_jvp(_device) and
 * bpltv_weighted_unrolled_gauss_newton for the two models above, argument for argument.  The tangent (dx, dy) is carried beside
 * (x, y) through the same maxiter iterations, from dx = df, dy = 0, on the step table of gamma = 0 (constant steps: nothing of
 * it depends on w, so nothing is omitted); the dual step and the projection's derivative are the weighted sweep's, and the
 * primal step's tangent is, with dv = dx - tau * G^T dy,
 *
 *     TV-L1:  dx+ = dv - tau * sign(x+ - f) * dw   where x+ != f or w = 0   (the threshold let the step through, or is the
 *             dx+ = df                             where x+ == f, w > 0      identity; a held pixel moves with f alone)
 *     TV-KL:  dx+ = (x+ * dv + tau w * df + tau (f - x+) * dw) / s,   1/s = x+ / (tau w f + x+^2);   dx+ = 0 where x+ = 0
 *
 * each decided on x+, f and w exactly as the model's reverse sweep decides it from the tape: the sweep is that VJP's transpose
 * pixel for pixel, <du, gu> = <df, grad_f> + <dalpha, grad_alpha> + <dw, grad_w>, and shares its conventions (TV-L1: the
 * derivative on the threshold's kink is the held side's; TV-KL: a clamped pixel passes nothing).  No tape: 16 planes of M*N*O
 * doubles, the weighted sweep's own workspace, whatever maxiter is.  u_out (may be NULL) is bpltv_lone_denoise's /
 * bpltv_kl_denoise's u bit for bit.  Everything else -- ndir directions one after the other, each bitwise the single call; NULL
 * tangents (not all three); finite tangents; the rejections, every one before anything of the handle changes; the last solve,
 * every tape and the solve statistics left as they were; no captured graph shared with any other call, the weighted sweep's
 * included; one shard forwarded, more BPLTV_E_UNSUPPORTED -- is bpltv_weighted_unrolled_jvp's contract.  TV-KL: the resident f
 * must be finite and >= 0 (BPLTV_E_ARG naming f; checked once per dataset).  stats: only adjoint_ms and adjoint_method = 17
 * (TV-L1) / 18 (TV-KL) change.
 * The two _gauss_newton calls: a scalar or a patch parameter of P = am*an <= 16 entries (a map or more: BPLTV_E_UNSUPPORTED;
 * use the model's _jvp for Jacobian columns), cost_out = 0.5||u_K - ubar||^2 on the resident ubar, grad_out = J^T (u_K - ubar),
 * hess_out = J^T J, as bpltv_weighted_unrolled_gauss_newton. */
int bpltv_lone_unrolled_jvp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                            const bpltv_params *p, int ndir, const double *df, const double *dalpha, const double *dw,
                            double *du_out, double *u_out /* may be NULL */);
int bpltv_lone_unrolled_jvp_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                   const bpltv_params *p, int ndir, const double *d_df, const double *d_dalpha,
                                   const double *d_dw, double *d_du, double *d_u /* may be NULL */);
int bpltv_lone_unrolled_gauss_newton(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                     const bpltv_params *p, double *cost_out, double *grad_out, double *hess_out);
int bpltv_kl_unrolled_jvp(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                          const bpltv_params *p, int ndir, const double *df, const double *dalpha, const double *dw,
                          double *du_out, double *u_out /* may be NULL */);
int bpltv_kl_unrolled_jvp_device(bpltv_t *h, const double *d_w, int wo, const double *d_alpha, int am, int an,
                                 const bpltv_params *p, int ndir, const double *d_df, const double *d_dalpha,
                                 const double *d_dw, double *d_du, double *d_u /* may be NULL */);
int bpltv_kl_unrolled_gauss_newton(bpltv_t *h, const double *w, int wo, const double *alpha, int am, int an,
                                   const bpltv_params *p, double *cost_out, double *grad_out, double *hess_out);

/* Forward mode through the channel-coupled iterations: bpltv_unrolled_jvp and
 * bpltv_unrolled_gauss_newton for the model above.  The tangent (dx, dy) is carried beside (x, y) through the same maxiter
 * iterations, from dx = df, dy = 0, with the step table held fixed; the derivative of the projection is taken per pixel of a
 * colour image over its planes, on the primal's own decision:
 *
 *     out:  q = rsqrt_nr(n2);  e_c = z_c*q;  dot = sum_c (e1_c*dz1_c + e2_c*dz2_c);  dy_c = dalpha*e_c + (alpha*q)*(dz_c - e_c*dot)
 *     else: dy_c = dz_c
 *
 * and du = dx after the last step: the exact transpose of bpltv_color_unrolled_vjp, <du, gu> = <df, grad_f> + <dalpha,
 * grad_alpha> to rounding.  No tape is read or written, so the memory does not grow with maxiter.
 *
 * bpltv_color_unrolled_jvp: ndir directions, one sweep each, one after the other.  df (ndir x M*N*O doubles) and dalpha
 * (ndir x am*an) are direction-major; either may be NULL (a zero tangent), not both (BPLTV_E_ARG); tangents must be finite.
 * du_out: ndir x M*N*O doubles.  u_out (may be NULL): bpltv_color_denoise's u, bit for bit.  Direction d of a call is bitwise
 * the call with that direction alone.  The _device form takes HBM addresses throughout (d_u may be NULL).
 * bpltv_color_unrolled_gauss_newton: for a scalar or a patch of P = am*an <= 16 entries (a map or a larger patch:
 * BPLTV_E_UNSUPPORTED) the cost 0.5 |u_K - ubar|^2 over all planes, grad_out = J^T (u_K - ubar) (P doubles) and hess_out =
 * J^T J (P x P, column major) from P unit-direction sweeps; bpltv_set_data's ubar is the target.
 *
 * The contract is bpltv_unrolled_jvp's with the colour solve's rules for channels and params: channels outside 1 ... 4 or not
 * dividing O, ndir < 1, maxiter < 1 and a bad parameter shape are BPLTV_E_ARG; rho, init and order must be 0
 * (BPLTV_E_UNSUPPORTED); no data is BPLTV_E_NODATA; every rejection comes before anything of the handle changes.  channels = 1
 * returns the bits of bpltv_unrolled_jvp.  The sweeps run in planes of the handle's own: the last solve, bpltv_u_device, the
 * colour tape and the TV tapes stay as they were, and of the statistics only adjoint_ms (the HIP-event time of the sweeps) and
 * adjoint_method = 13 change.  The results do not depend on tile_iters, on the launch chains, on use_graph or on the host or
 * device form.  Multi-device handles behave as for bpltv_unrolled_jvp. */
int bpltv_color_unrolled_jvp(bpltv_t *h, int channels, const double *alpha, int am, int an, const bpltv_params *p, int ndir,
                             const double *df, const double *dalpha, double *du_out, double *u_out /* may be NULL */);
int bpltv_color_unrolled_jvp_device(bpltv_t *h, int channels, const double *d_alpha, int am, int an, const bpltv_params *p,
                                    int ndir, const double *d_df, const double *d_dalpha, double *d_du, double *d_u);
int bpltv_color_unrolled_gauss_newton(bpltv_t *h, int channels, const double *alpha, int am, int an, const bpltv_params *p,
                                      double *cost_out, double *grad_out, double *hess_out);

/* Jacobian-vector product of u = denoise(f, alpha) (TV model): du for tangents (df, dalpha), defined as the linear map
 * whose transpose bpltv_vjp computes, in every branch -- <gu, du> = <grad_f(gu), df> + <grad_alpha(gu), dalpha> for any
 * gu -- so forward and reverse mode agree, also where the reference's linearisation is not the true one (reg = 1 with an
 * array parameter).  With G the forward-difference gradient, h the per-pixel plane of the gradient's last step and up()
 * the patch upsampling, one direction solves the system bpltv_vjp factors with
 *     reg = 0, and reg = 1 with a scalar:    r = df - G^T (h o up(dalpha)),    A q = r,      du = q
 *     reg = 1 with a patch or map:           r = df - (G^T h) o up(dalpha),    A_s q = S r,  du = S^-1 q,  S = diag(sqrt(alpha)).
 * For reg = 0 this is the derivative of the solution map itself (active set held fixed).
 * ndir >= 1 directions, direction-major, are solved against ONE factorisation per image group: df is NULL or
 * ndir * M*N*O doubles, dalpha NULL or ndir * am*an doubles, not both NULL (a NULL tangent is zero); du_out: ndir * M*N*O
 * doubles, direction d of a call being bitwise the ndir = 1 call with that direction.  The contract is bpltv_vjp's:
 * alpha is checked as bpltv_denoise checks it (finite, >= 0; > 0 for reg = 1 with an array parameter) and the tangents
 * must be finite; ndir < 1 or both tangents NULL is BPLTV_E_ARG; every rejection comes before anything of the handle
 * changes.  The parameter is staged apart: the last solve, bpltv_u_device, bpltv_duality_gap and the captured graphs stay
 * as they were.  The residual gate and the kappa retry apply; stats report the adjoint, adjoint_residual being the worst
 * over the directions.  dtype = 32 handles too; no dataset is needed; image groups ("adjoint_budget_mb") give bitwise the
 * same result.  Multi-device handles split the images as bpltv_vjp does and write the du slices in place. */
int bpltv_jvp(bpltv_t *h, const double *u, const double *alpha, int am, int an, int reg, const bpltv_params *p,
              int ndir, const double *df, const double *dalpha, double *du_out);
/* The same with every array in HBM (device pointers); parameter and tangents are checked on the device.  Single-device
 * handles (multi: BPLTV_E_UNSUPPORTED beyond one shard). */
int bpltv_jvp_device(bpltv_t *h, const double *d_u, const double *d_alpha, int am, int an, int reg,
                     const bpltv_params *p, int ndir, const double *d_df, const double *d_dalpha, double *d_du);
/* One parameter per image (the forward mode of bpltv_vjp_each): alphas holds O blocks of am x an doubles, dalphas
 * ndir x O blocks (direction, then image).  Image k reads its own blocks; its du is bitwise what a one-image handle
 * returns for block k. */
int bpltv_jvp_each(bpltv_t *h, const double *u, const double *alphas, int am, int an, int reg, const bpltv_params *p,
                   int ndir, const double *df, const double *dalphas, double *du_out);
int bpltv_jvp_each_device(bpltv_t *h, const double *d_u, const double *d_alphas, int am, int an, int reg,
                          const bpltv_params *p, int ndir, const double *d_df, const double *d_dalphas, double *d_du);

/* Gauss-Newton model of the loss 0.5||u(alpha) - ubar||^2 for one shared parameter (TV model): with J the M*N*O x P
 * matrix of the columns du/dalpha_j (P = am*an; the unit directions of bpltv_jvp against one factorisation),
 *     hess_out = J^T J   (P x P doubles, column major, symmetric bit for bit),     grad_out = J^T (u - ubar)   (P doubles),
 * grad_out being bpltv_gradient's result up to rounding (the transpose identity).  A scalar or a patch parameter with
 * P <= 16; a larger patch or a pixel map: BPLTV_E_UNSUPPORTED.  The columns live in a workspace of P * M*N*O doubles
 * (BPLTV_E_NOMEM if it does not fit).  Sums run per image, then over the images in image order (reproducible);
 * multi-device handles add the shards' [grad, H] on the host in shard order.  Checks, staging and stats as bpltv_jvp. */
int bpltv_gauss_newton(bpltv_t *h, const double *u, const double *ubar, const double *alpha, int am, int an, int reg,
                       const bpltv_params *p, double *grad_out, double *hess_out);

/* Vector-Jacobian product of u = sumregs_denoise(f, x) for a cotangent gu = dL/du: the adjoint system of
 * bpltv_sumregs_evaluate's gradient with the right-hand side
 *     reg = 0 (sumregs_gradient):      gu        grad_f_out =  p
 *     reg = 1 (sumregs_gradient_reg): -gu        grad_f_out = -p
 * solved once for the adjoint state p; grad_alpha_out = the parameter gradient computed from the same p.  So
 * gu = u - ubar gives bitwise the grad_out of bpltv_sumregs_evaluate (reg = !(delta > delta_t)) on the same u.
 * With reg = 1 and a patch or map parameter the reference's system I + sum_k diag(x_k) K_k is row-scaled, not
 * symmetric, and its gradient uses A^-1, not A^-T: both outputs follow it, so grad_f_out is
 * then not the transpose of the forward linearisation.  Such a parameter needs every entry > 0.
 * Argument lists as bpltv_vjp's; alpha and grad_alpha_out: 3*am*an doubles in bpltv_sumregs_evaluate's layout.  alpha
 * is checked as bpltv_sumregs_denoise checks it (finite, >= 0), gu must be finite; params.reserved[4] = 2 (block
 * cyclic reduction) returns BPLTV_E_UNSUPPORTED.  Every rejection comes before anything of the handle changes.  The
 * parameter is staged apart: the last solve, bpltv_u_device, bpltv_duality_gap and the captured graphs stay as they
 * were (bpltv_per_image does not).  stats report the adjoint.  dtype = 32 handles too (the model is Float64 there).
 * Multi-device handles split the images as bpltv_vjp does. */
int bpltv_sumregs_vjp(bpltv_t *h, const double *u, const double *alpha, int am, int an, int reg, const bpltv_params *p,
                      const double *gu, double *grad_f_out, double *grad_alpha_out);
/* The same with every array in HBM; the parameter and the cotangent are checked on the device.  Single-device handles
 * (multi: BPLTV_E_UNSUPPORTED beyond one shard). */
int bpltv_sumregs_vjp_device(bpltv_t *h, const double *d_u, const double *d_alpha, int am, int an, int reg,
                             const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alpha);

/* One parameter block per image for the sum-of-regularisers model: what bpltv_denoise_each and its family are to the TV
 * model.  alphas: O blocks of 3*am*an doubles, block k at alphas + k*3*am*an, each in bpltv_sumregs_evaluate's layout
 * (three slices of am x an, column major, forward / backward / centred).  u_k is bitwise what a one-image handle returns
 * for (f_k, block k).  Each function keeps the contract of its twin (bpltv_sumregs_denoise, bpltv_sumregs_denoise_device,
 * bpltv_sumregs_vjp, bpltv_sumregs_vjp_device), word for word: every entry of every block is checked (finite, >= 0; > 0
 * when params.rho != 0, and for reg = 1 with a patch or map parameter) and gu must be finite before anything of the
 * handle changes; params.reserved[4] = 2 and params.init / params.order return BPLTV_E_UNSUPPORTED; dtype = 32 handles
 * work (the model is Float64 there); check_every / gap_tol and bpltv_duality_gap use image k's own block; a shared and
 * a per-image solve on one handle never replay each other's captured graphs; the VJP leaves the last solve,
 * bpltv_u_device, bpltv_duality_gap and the graphs untouched, and the kappa retry and the residual gate apply to it.
 * grad_f_out is bpltv_sumregs_vjp's; grad_alphas_out receives O blocks in the layout of alphas, block k = image k's
 * term alone (their sum in image order is bitwise bpltv_sumregs_vjp's grad_alpha_out when all blocks are equal).
 * Multi-device handles hand shard k the blocks [lo_k, hi_k) and write its gradient blocks in place; the device forms
 * return BPLTV_E_UNSUPPORTED beyond one shard.  bpltv_sumregs_evaluate and bpltv_sumregs_sweep take one block for the
 * batch: their sums over the images define the reference's learning function. */
int bpltv_sumregs_denoise_each(bpltv_t *h, const double *alphas, int am, int an, const bpltv_params *p, double *u_out);
int bpltv_sumregs_denoise_each_device(bpltv_t *h, const double *d_alphas, int am, int an, const bpltv_params *p);
int bpltv_sumregs_vjp_each(bpltv_t *h, const double *u, const double *alphas, int am, int an, int reg,
                           const bpltv_params *p, const double *gu, double *grad_f_out, double *grad_alphas_out);
int bpltv_sumregs_vjp_each_device(bpltv_t *h, const double *d_u, const double *d_alphas, int am, int an, int reg,
                                  const bpltv_params *p, const double *d_gu, double *d_grad_f, double *d_grad_alphas);

/* Jacobian-vector product of u = sumregs_denoise(f, x): du for tangents (df, dx), defined as the linear map whose
 * transpose bpltv_sumregs_vjp computes, in every branch -- <gu, du> = <grad_f(gu), df> + <grad_alpha(gu), dx> for any gu.
 * With h_k the per-element planes of the gradient's last step (k = forward, backward, centred), w_k = G_k^T h_k per node,
 * up() the patch upsampling and A the matrix bpltv_sumregs_vjp factors for the same (u, x, reg), one direction is
 *     r = df - sum_k w_k o up(dx_k)   (a vector parameter: dx_k a scalar),      du = A^-T r.
 * A^T = A except for reg = 1 with a patch or map parameter, whose row-scaled system is not symmetric: there
 * A^T = I + sum_k K_k diag(up(x_k)), factored as such.  There is no sign: the VJP's -gu / -p pair for reg = 1 cancels.
 * alpha / dalpha use bpltv_sumregs_evaluate's layout (three slices of am x an); dalpha holds ndir blocks of 3*am*an
 * doubles, df ndir * M*N*O doubles, either may be NULL (a zero tangent), not both; du_out: ndir * M*N*O doubles.  The
 * ndir >= 1 directions are solved against ONE factorisation per image group, direction d of a call being bitwise the
 * ndir = 1 call with that direction.  The contract is bpltv_jvp's and bpltv_sumregs_vjp's: the parameter must be finite
 * and >= 0 (> 0 for reg = 1 with an array parameter), the tangents finite; ndir < 1 or both tangents NULL is
 * BPLTV_E_ARG, params.reserved[4] = 2 BPLTV_E_UNSUPPORTED; every rejection comes before anything of the handle changes,
 * and the last solve, bpltv_u_device, bpltv_duality_gap and the captured graphs stay as they were.  The kappa retry and
 * the residual gate apply (the gate takes the worst direction); stats report the adjoint.  dtype = 32 handles too; image
 * groups ("adjoint_budget_mb") give bitwise the same result.  Multi-device handles split the images as bpltv_jvp does. */
int bpltv_sumregs_jvp(bpltv_t *h, const double *u, const double *alpha, int am, int an, int reg, const bpltv_params *p,
                      int ndir, const double *df, const double *dalpha, double *du_out);
/* The same with every array in HBM; parameter and tangents are checked on the device.  Single-device handles (multi:
 * BPLTV_E_UNSUPPORTED beyond one shard). */
int bpltv_sumregs_jvp_device(bpltv_t *h, const double *d_u, const double *d_alpha, int am, int an, int reg,
                             const bpltv_params *p, int ndir, const double *d_df, const double *d_dalpha, double *d_du);
/* One parameter block per image (the forward mode of bpltv_sumregs_vjp_each): alphas holds O blocks of 3*am*an doubles,
 * dalphas ndir x O blocks (direction, then image).  Image k reads its own blocks; its du is bitwise what a one-image
 * handle returns for block k. */
int bpltv_sumregs_jvp_each(bpltv_t *h, const double *u, const double *alphas, int am, int an, int reg,
                           const bpltv_params *p, int ndir, const double *df, const double *dalphas, double *du_out);
int bpltv_sumregs_jvp_each_device(bpltv_t *h, const double *d_u, const double *d_alphas, int am, int an, int reg,
                                  const bpltv_params *p, int ndir, const double *d_df, const double *d_dalphas,
                                  double *d_du);

/* Gauss-Newton model of 0.5||u(x) - ubar||^2 for one shared parameter of the sum-of-regularisers model: with J the
 * M*N*O x P matrix of the columns du/dx_j (P = 3*am*an, ordered as the parameter layout; the unit directions of
 * bpltv_sumregs_jvp against one factorisation),
 *     hess_out = J^T J   (P x P doubles, column major, symmetric bit for bit),     grad_out = J^T (u - ubar)   (P doubles).
 * P <= 16: a vector, or a patch up to 2 x 2 (or 1 x 5); larger patches and pixel maps: BPLTV_E_UNSUPPORTED.  Sums run per
 * image, then over the images in image order; multi-device handles add the shards' [grad, H] on the host in shard
 * order.  Checks, staging and stats as bpltv_sumregs_jvp. */
int bpltv_sumregs_gauss_newton(bpltv_t *h, const double *u, const double *ubar, const double *alpha, int am, int an,
                               int reg, const bpltv_params *p, double *grad_out, double *hess_out);

/* Forward-only parameter sweep: generate_cost / generate_2d_cost (src/BPLDenoising.jl:92-111,
 * :136-158) evaluate cost(alpha_k) = 0.5*||TVDenoise(f, alpha_k) - ubar||^2 for a range of parameters,
 * one solve after the other.  Here the K parameter blocks (each am x an, column major, K*am*an
 * doubles) times the O resident images form ONE batch of K*O independent ROF problems -- the second
 * data-parallel axis that fills a GPU even with a single image.  cost_out: K doubles; u_out: NULL
 * or K*M*N*O doubles (parameter-major).  Use maxiter = 10000 for the TVDenoise setting.  Every entry must be finite
 * and >= 0, and > 0 when p->rho != 0; a rejected call (those entries, the kernel plan, p->init / p->order on a dtype = 32
 * handle) returns an error and leaves the handle as it was.  check_every / gap_tol are ignored (maxiter iterations).  The
 * blocks live in a parameter buffer of the sweep's own, so the last solve's result (bpltv_u_device, bpltv_duality_gap)
 * stays that of the last denoise / evaluate.
 * Multi-device handles split whichever axis leaves the smaller largest share per device: the images (device k solves
 * K x O_k problems on the shard it already holds) or the K parameter blocks (device r solves K_r x O problems on a
 * REPLICA -- a second, whole copy of the dataset made on every requested device at the first such sweep, filled from
 * the shards' resident data).  With the reference's default num_samples = 1 (src/BPLDenoising.jl:313) or the one-pair
 * sets (datasets/cameraman_128_10/filelist.txt) only the parameter axis can use more than one GPU: 100 parameters x 1
 * image on 8 devices = 13,13,13,13,12,12,12,12 problems per device.  Costs are concatenated (every replica sums over
 * all O images in image order), u_out slices are written in place: the results are bitwise those of one single-device
 * handle either way.  bpltv_set_option "sweep_split" (0 automatic, 1 images, 2 parameters) forces an axis;
 * stats.sweep_shards = devices the parameter blocks were split over (0: image split / single device). */
int bpltv_sweep(bpltv_t *h, const double *alphas, int K, int am, int an, const bpltv_params *p,
                double *cost_out, double *u_out);

/* The same sweep for the sum-of-regularisers model: generate_cost / generate_2d_cost (src/BPLDenoising.jl:92-158) with
 * denoise_function = sumregs_denoise (src/SumRegsLearningFunction.jl:38-85).  alphas: K blocks of 3*am*an doubles, each
 * in the layout bpltv_sumregs_evaluate takes; p = NULL: bpltv_sumregs_default_params.  cost_out: K doubles; u_out: NULL
 * or K*M*N*O doubles (parameter-major).  Every entry must be finite and >= 0, and > 0 when p->rho != 0; a rejected call
 * returns BPLTV_E_ARG and leaves the handle as it was.  check_every / gap_tol are ignored (maxiter iterations, as in
 * bpltv_sweep).  The K*O problems run in groups of whole parameter blocks: at most 65535 problems per group (a grid
 * dimension) and what fits in HBM (14 planes of M*N doubles per problem; option "sr_sweep_budget_mb"), with bitwise the
 * same result for any grouping (stats.sweep_groups).  The last solve's result (bpltv_u_device, bpltv_duality_gap) stays
 * that of the last denoise / evaluate.  Multi-device handles split the images or the parameter blocks as bpltv_sweep does;
 * the parameter split is bitwise a single handle's result, the image split adds per-shard partial costs on the host and
 * agrees to rounding. */
int bpltv_sumregs_sweep(bpltv_t *h, const double *alphas, int K, int am, int an, const bpltv_params *p,
                        double *cost_out, double *u_out);

/* Handle options: aids for tests and measurements, none of them changes a result or is needed for the reference's
 * behaviour (the reference has no counterpart; its sparse `\` at src/TVLearningFunctionVec.jl:131,248 has no knobs).
 * They replace the environment variables earlier versions read on the product path.  Unknown names: BPLTV_E_ARG.
 *   "adjoint_budget_mb"  > 0: HBM (MB) the adjoint's factor workspace may take -- forces the gradient to run in image
 *                        groups (stats.adjoint_chunks; bitwise the same result); 0 = what is free minus a 2 GB reserve
 *   "sr_force_lu"        1: sum of regularisers -- factor the symmetric systems by the LU variant of the nested
 *                        dissection as well (cross-check of that variant)
 *   "nd_leaf"            leaf size in pixels of the nested-dissection tree (0 = 32)
 *   "nd_wave"            0: fronts of <= 64 rows are factored by the workgroup-per-front kernel like the larger small fronts
 *                        (cross-check of the wave-per-front kernel, which is the default: 1)
 *   "nd_skinny"          0: fronts of <= 32 pivots that keep only their pivot block columns in LDS go through the older
 *                        kernels instead (cross-check; default 1)
 *   "nd_skinny_min", "nd_skinny2_min"   (front, image) pairs a level needs before those two kernels take it (defaults 0 / 256:
 *                        below that the five short launches of the large regime finish a level sooner than one long one)
 *   "nd_staged"          0: substitutions of the small levels by the column-loop kernels (cross-check: the same bits; default 1)
 *   "hb_sync"            HBM band cross-check solver (params.reserved[4] = 1): 0 automatic, 1 HIP events (what a
 *                        rocprofv3 run needs), 2 stream memory operations (BPLTV_E_HIP when the device has none)
 *   "hb_single_stream"   1: that solver's three streams folded into one (rocprofv3 --pmc)
 *   "hb_rw"              32 | 128: rows per workgroup of its substitutions (0 = by size)
 *   "sr_sweep_budget_mb" > 0: HBM (MB) the state of bpltv_sumregs_sweep may take -- forces groups of parameter blocks
 *                        (stats.sweep_groups; bitwise the same result); 0 = what is free minus a 2 GB reserve
 *   "sweep_split"        multi-device handles, bpltv_sweep / bpltv_sumregs_sweep: 0 automatic, 1 split the images, 2 split
 *                        the parameter blocks
 *   "tape_checkpoint"    the unrolled solves and sweeps of the four models, the channel-coupled one included (see bpltv_unrolled_tape_doubles): 0 the full tape,
 *                        C >= 1 the iteration state every C iterations instead (the sweep recomputes each segment's tape: the
 *                        same bits, one more forward solve), -1 the spacing of least memory.  A value that is no integer or
 *                        lies below -1 is BPLTV_E_ARG and the option keeps its value.  The one option that is no test aid:
 *                        bpltv_params cannot grow
 * Multi-device handles pass the other options to every shard (and sweep replica). */
int bpltv_set_option(bpltv_t *h, const char *name, double value);

int bpltv_stats(bpltv_t *h, bpltv_stats_t *out);
const char *bpltv_last_error(bpltv_t *h);
int bpltv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BPLTV_H */
