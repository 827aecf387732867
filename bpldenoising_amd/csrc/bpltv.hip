// bpltv.hip -- libbpltv: handle, launch logic and the C ABI declared in include/bpltv.h.
//
// Drop-in boundary: /root/reference/src/TVLearningFunctionVec.jl:14-27 (tv_op_learning_function),
// :45-70 (denoise), /root/reference/src/BPLDenoising.jl:41-82 (TVDenoise).  The product path is
// GPU only: there is no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/bpltv.h"
#include "adjoint_hbm_kernels.hpp"
#include "hb_band_solver.hpp"
#include "hb_lu_solver.hpp"
#include <thread>
#include "nd_solver.hpp"
#include "adjoint_bcr_kernels.hpp"
#include "adjoint_kernels.hpp"
#include "pdhg_kernels.hpp"
#include "sumregs_kernels.hpp"
#include "weighted_kernels.hpp"
#include "tv_tile_kernels.hpp"
#include "color_tile_kernels.hpp"
#include "sumregs_unrolled_kernels.hpp"
#include "multi_gpu.hpp"

using namespace bpltv;

namespace {

// ------------------------------------------------------------------------------------------
// PDHG kernel variants: (PI, PJ) pixels per thread, (TI, TJ) threads; region = PI*TI x PJ*TJ.
// ------------------------------------------------------------------------------------------
struct Variant {
    int RI, RJ, threads;
    void (*launch)(const PdhgArgs&, int grid, hipStream_t);
    const void* func;  // kernel symbol, for hipGraphAddKernelNode
    size_t lds;
    const char* name;
    // the single-precision instantiation (handles created with dtype = 32)
    void (*launch32)(const PdhgArgs&, int grid, hipStream_t);
    const void* func32;
    size_t lds32;
    int tiles_per_block;   // 1: one workgroup per tile (pdhg_tile_kernel); > 1: that many one-wave tiles per workgroup
    int min_image;         // 1: the image must be at least as large as the region (pdhg_rows_kernel); 2: at least as wide
    int tmax = 0;          // > 0: most iterations a launch can fuse (pdhg_stream_kernel)
    // pdhg_tile_kernel only: func / func32 are compiled for the (nTi, nTj, images) grid, these for the 1-D grid
    const void* func_1d = nullptr;
    const void* func32_1d = nullptr;
};
// the kernel symbol of a launch of variant V: the tile kernels know the form of their grid when they are compiled
// fast: PdhgArgs::fast of the launch (pdhg_fill_invariants) -- the FAST instantiation of variant 1, 3-D grid
inline const void* pdhg_func(const Variant& V, int dtype, int grid3d, int fast) {
    if (fast)
        return dtype == 32 ? reinterpret_cast<const void*>(&pdhg_tile_kernel<float, 1, 1, 32, 32, true, true>)
                           : reinterpret_cast<const void*>(&pdhg_tile_kernel<double, 1, 1, 32, 32, true, true>);
    if (!grid3d && V.func_1d) return dtype == 32 ? V.func32_1d : V.func_1d;
    return dtype == 32 ? V.func32 : V.func;
}

// grid of a launch of `tiles` tiles: (nTi, nTj, images) when the kernel decodes blockIdx that way (PdhgArgs::grid3d)
inline dim3 pdhg_grid(const PdhgArgs& a, int tiles) {
    return a.grid3d ? dim3(a.nTi, a.nTj, tiles / (a.nTi * a.nTj)) : dim3(tiles);
}
// whether a launch of `nimg` images can use the 3-D grid (one tile per workgroup, grid.y / grid.z limits)
inline int pdhg_grid3d_ok(int nTj, int nimg, int tiles_per_block) { return (tiles_per_block == 1 && nTj <= 65535 && nimg <= 65535) ? 1 : 0; }

template <typename T, int PI, int PJ, int TI, int TJ>
void launch_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    constexpr size_t lds = pdhg_lds_bytes(PI * TI, PJ * TJ, sizeof(T));
    if constexpr (PI == 1 && PJ == 1 && TI == 32 && TJ == 32) {
        if (a.fast) {
            hipLaunchKernelGGL((pdhg_tile_kernel<T, PI, PJ, TI, TJ, true, true>), pdhg_grid(a, grid), dim3(TI * TJ), lds, s, a);
            return;
        }
    }
    if (a.grid3d) hipLaunchKernelGGL((pdhg_tile_kernel<T, PI, PJ, TI, TJ, true>), pdhg_grid(a, grid), dim3(TI * TJ), lds, s, a);
    else hipLaunchKernelGGL((pdhg_tile_kernel<T, PI, PJ, TI, TJ, false>), pdhg_grid(a, grid), dim3(TI * TJ), lds, s, a);
}

#define VAR(PI, PJ, TI, TJ)                                                                    \
    { PI * TI, PJ * TJ, TI * TJ, &launch_variant<double, PI, PJ, TI, TJ>,                       \
      reinterpret_cast<const void*>(&pdhg_tile_kernel<double, PI, PJ, TI, TJ, true>),           \
      pdhg_lds_bytes(PI * TI, PJ * TJ), #PI "x" #PJ "px_" #TI "x" #TJ "thr",                    \
      &launch_variant<float, PI, PJ, TI, TJ>,                                                   \
      reinterpret_cast<const void*>(&pdhg_tile_kernel<float, PI, PJ, TI, TJ, true>),            \
      pdhg_lds_bytes(PI * TI, PJ * TJ, sizeof(float)), 1, 0, 0,                                 \
      reinterpret_cast<const void*>(&pdhg_tile_kernel<double, PI, PJ, TI, TJ, false>),          \
      reinterpret_cast<const void*>(&pdhg_tile_kernel<float, PI, PJ, TI, TJ, false>) }
// register tiles: one wave per 32 x (2 PJ) region, WPB waves per workgroup (pdhg_wave_kernel)
template <typename T, int PJ, int WPB>
void launch_wave_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pdhg_wave_kernel<T, PJ, WPB>), dim3((grid + WPB - 1) / WPB), dim3(64 * WPB), 0, s, a);
}
#define VARW(PJ, WPB)                                                                           \
    { 32, 2 * PJ, 64 * WPB, &launch_wave_variant<double, PJ, WPB>,                              \
      reinterpret_cast<const void*>(&pdhg_wave_kernel<double, PJ, WPB>), 0, "wave_32x" #PJ "x2",  \
      &launch_wave_variant<float, PJ, WPB>,                                                     \
      reinterpret_cast<const void*>(&pdhg_wave_kernel<float, PJ, WPB>), 0, WPB, 0 }
// 64-lane rows, PJ pixels per thread along j, TJ waves (pdhg_rows_kernel): region 64 x (PJ * TJ); CL: f and alpha in LDS
template <typename T, int PJ, int TJ, bool CL>
void launch_rows_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pdhg_rows_kernel<T, PJ, TJ, CL>), pdhg_grid(a, grid), dim3(64 * TJ), pdhg_rows_lds(PJ, TJ, CL, sizeof(T)), s, a);
}
#define VARR(PJ, TJ, CL)                                                                        \
    { 64, PJ * TJ, 64 * TJ, &launch_rows_variant<double, PJ, TJ, CL>,                           \
      reinterpret_cast<const void*>(&pdhg_rows_kernel<double, PJ, TJ, CL>), pdhg_rows_lds(PJ, TJ, CL),  \
      "rows_64x" #PJ "px_" #TJ "waves" #CL, &launch_rows_variant<float, PJ, TJ, CL>,            \
      reinterpret_cast<const void*>(&pdhg_rows_kernel<float, PJ, TJ, CL>), pdhg_rows_lds(PJ, TJ, CL, sizeof(float)), 1, 1 }
// rows of 128 pixels, two waves side by side (pdhg_rowsw_kernel): region 128 x (PJ * TJ), 128 * TJ threads
template <typename T, int PJ, int TJ>
void launch_rowsw_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pdhg_rowsw_kernel<T, PJ, TJ>), pdhg_grid(a, grid), dim3(128 * TJ), pdhg_rowsw_lds(PJ, TJ, sizeof(T)), s, a);
}
#define VARRW(PJ, TJ)                                                                           \
    { 128, PJ * TJ, 128 * TJ, &launch_rowsw_variant<double, PJ, TJ>,                            \
      reinterpret_cast<const void*>(&pdhg_rowsw_kernel<double, PJ, TJ>), pdhg_rowsw_lds(PJ, TJ), \
      "rows_128x" #PJ "px_" #TJ "strips", &launch_rowsw_variant<float, PJ, TJ>,                 \
      reinterpret_cast<const void*>(&pdhg_rowsw_kernel<float, PJ, TJ>), pdhg_rowsw_lds(PJ, TJ, sizeof(float)), 1, 1 }
// the same re-cut for instruction-level parallelism (pdhg_rows2_kernel): G dual chains of an interior wave in flight
template <typename T, int PJ, int TJ, int G>
void launch_rows2_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pdhg_rows2_kernel<T, PJ, TJ, G>), pdhg_grid(a, grid), dim3(64 * TJ), pdhg_rows2_lds(PJ, TJ, sizeof(T)), s, a);
}
#define VARR2(PJ, TJ, G)                                                                        \
    { 64, PJ * TJ, 64 * TJ, &launch_rows2_variant<double, PJ, TJ, G>,                           \
      reinterpret_cast<const void*>(&pdhg_rows2_kernel<double, PJ, TJ, G>), pdhg_rows2_lds(PJ, TJ),  \
      "rows2_64x" #PJ "px_" #TJ "waves_g" #G, &launch_rows2_variant<float, PJ, TJ, G>,          \
      reinterpret_cast<const void*>(&pdhg_rows2_kernel<float, PJ, TJ, G>), pdhg_rows2_lds(PJ, TJ, sizeof(float)), 1, 1 }
// a pipeline of waves streaming down a 64-column strip (pdhg_stream_kernel): SEG rows per segment core, NL levels
template <typename T, int NL, int D, int FD, int PF, int WPE>
void launch_stream_variant(const PdhgArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pdhg_stream_kernel<T, NL, D, FD, PF, WPE>), pdhg_grid(a, grid), dim3(64 * NL), (pdhg_stream_lds<NL, D, FD>(sizeof(T))), s, a);
}
#define VARS(SEG, NL, D, FD, PF, WPE)                                                               \
    { 64, SEG + 2 * NL, 64 * NL, &launch_stream_variant<double, NL, D, FD, PF, WPE>,                  \
      reinterpret_cast<const void*>(&pdhg_stream_kernel<double, NL, D, FD, PF, WPE>), pdhg_stream_lds<NL, D, FD>(),  \
      "stream_64x" #SEG "rows_" #NL "levels_d" #D, &launch_stream_variant<float, NL, D, FD, PF, WPE>, \
      reinterpret_cast<const void*>(&pdhg_stream_kernel<float, NL, D, FD, PF, WPE>), pdhg_stream_lds<NL, D, FD>(sizeof(float)), 1, 2, NL }
const Variant kVariants[] = {
    VAR(1, 1, 32, 32),  // 1: 32x32 region, 1 px/thread   (small images, shallow blocking).  Besides the general instantiations
                        //    of both grid forms, this variant alone has pdhg_tile_kernel<double / float, 1, 1, 32, 32, true, true>:
                        //    FAST, the 3-D grid, for solves without sweep and rho with a scalar or full-map alpha (pdhg_func)
    VAR(2, 2, 32, 32),  // 2: 64x64 region, 4 px/thread
    VAR(1, 1, 16, 16),  // 3: 16x16 region
    VAR(2, 2, 16, 16),  // 4: 32x32 region, 256 threads
    VAR(2, 1, 32, 32),  // 5: 64x32 region
    VAR(4, 4, 16, 16),  // 6: 64x64 region, 256 threads, 16 px/thread
    VAR(1, 1, 64, 16),  // 7: 64x16 region (512 B rows)
    VAR(2, 1, 64, 16),  // 8: 128x16 region
    VAR(2, 2, 64, 16),  // 9: 128x32 region
    VAR(1, 2, 32, 32),  // 10: 32x64 region
    VAR(1, 2, 40, 20),  // 11: 40x40 region, 800 threads, 2 px/thread (core 24 at T = 8: 5x5 tiles per 128^2 image)
    VAR(2, 2, 20, 20),  // 12: 40x40 region, 400 threads, 4 px/thread
    VAR(1, 3, 48, 16),  // 13: 48x48 region, 768 threads, 3 px/thread   (default for images larger than 256)
    VAR(3, 2, 32, 32),  // 14: 96x64 region, 1024 threads, 6 px/thread: 150 KB of LDS, redundancy 1.60 at T = 8
    VAR(2, 3, 48, 16),  // 15: 96x48 region, 768 threads, 6 px/thread: 112 KB of LDS, redundancy 1.80 at T = 8
    VARW(16, 4),        // 16: register tiles, one wave per 32x32 region (16 px per lane), no LDS, no barriers
    VARW(8, 4),         // 17: ... per 32x16 region (8 px per lane)
    VARW(12, 4),        // 18: ... per 32x24 region (12 px per lane)
    VARR(8, 8, false),  // 19: 64-lane rows, 64x64 region, 8 px per thread, 512 threads
    VARR(6, 8, false),  // 20: ... 64x48 region, 6 px per thread
    VARR(8, 16, false), // 21: ... 64x128 region, 8 px per thread, 1024 threads
    VARR(4, 16, false), // 22: ... 64x64 region, 4 px per thread, 1024 threads
    VARR(6, 16, false), // 23: ... 64x96 region, 6 px per thread, 1024 threads
    VARR(8, 8, true),   // 24: as 19 with f and alpha in LDS
    VARR(6, 8, true),   // 25: as 20 ...
    VARR(10, 8, true),  // 26: 64x80 region, 10 px per thread, 512 threads
    VARR(12, 8, true),  // 27: 64x96 region, 12 px per thread, 512 threads
    VARR(12, 4, true),  // 28: 64x48 region, 12 px per thread, 256 threads
    VARR(16, 4, true),  // 29: 64x64 region, 16 px per thread, 256 threads
    VARR2(8, 8, 1),     // 30: rows2, 64x64 region, 8 px per thread; one dual chain at a time (the trims alone)
    VARR2(8, 8, 2),     // 31: ... two dual chains in flight
    VARS(256, 8, 4, 32, 2, 4),   // 32: streaming pipeline of 8 waves, segments of 256 rows, rings of 4 rows (76 KB of LDS), 128 VGPRs: two workgroups per CU
    VARS(256, 8, 2, 16, 2, 6),   // 33: ... rings of 2 rows (38 KB), 80 VGPRs: three workgroups per CU
    VARRW(8, 8),        // 34: rows of 128 pixels (two waves side by side), 128x64 region, 8 px per thread, 1024 threads
    VARRW(8, 4),        // 35: ... 128x32 region, 512 threads
    VARRW(6, 8),        // 36: ... 128x48 region, 6 px per thread, 1024 threads
    // (round 4, 8 x 1024^2 pixel map, 480 iterations: 32 / 33 run 2.9-3.0e4 / 3.2-3.3e4 it/s against 4.1-4.2e4 of variant 19; four or
    //  six rows of prefetch (spills) 3.0e4; segments of 128 / 352 / 512 rows 3.2e4 / 3.0e4 / 2.2e4; the same pipeline fed by a
    //  loader wave through LDS-DMA 2.2-3.3e4 -- DESIGN.md section 4.1)
    // (round 4, 8 x 1024^2 pixel map, 480 iterations: variant 19 4.09-4.22e4 it/s, 30 4.09-4.15e4, 31 4.02e4, four chains
    //  3.83e4 (spills); 64x48 / 6 px with two or three chains 3.51e4 against variant 20's 3.58e4 -- fewer moves and more
    //  chains in flight buy nothing: DESIGN.md section 4.1)
    // (64x36 / 3 px and 64x48 / 4 px with 64-thread rows -- whole halo waves that stop early -- were measured too: 86
    //  resp. 110 VGPRs, one workgroup per CU, 1.88e4 / 2.14e4 it/s on 8 x 1024^2 against 2.55e4 for variant 13)
    // (64x48 / 3 px, 48x48 / 4 px, 56x54 / 3 px, 48x48 with the 3 px along i, 64x32 / 2 px were measured on
    //  8 x 1024^2 as well: none beats variant 13)
};

// The models whose solves the shared launch driver (run_chains) runs
enum Model { MODEL_TV = 0, MODEL_SR = 1, MODEL_W = 2, MODEL_UN = 3, MODEL_SRUN = 4, MODEL_COLOR = 5, NMODELS = 6 };   // MODEL_UN: the taped solve, its reverse sweep and the tangent sweep
                                                                                                     // MODEL_SRUN: the same of the sum-of-regularisers model
                                                                                                     // MODEL_COLOR: the solves, the reverse sweep and the tangent sweep of the channel-coupled model

// What identifies a launch sequence built into graphs: everything its kernel arguments and its cut into launches depend
// on.  One key type for all models (a field a model does not use stays 0); each model has a cache of its own
// (bpltv_handle::graphs), so a weighted and an unweighted solve never replay each other's graphs.
struct GraphKey {
    int maxiter, T, variant, am, an, chains;
    double rho, tau0, sigma0;
    int accel, dbg, nimg;
    const void* state; // state set 0 of the solve context: a sweep never replays a dataset-context graph, nor the reverse
                       // (MODEL_UN: the tape the launches write or read, with variant 0 = taped solve, 1 = reverse sweep; 2 ... 5 = tangent
                       // sweep, whose planes stand here instead; 6 = weighted taped solve, 7 / 8 = its reverse sweep without / with grad_w,
                       // 9 ... 16 = its tangent sweep, by the tangents it reads, its planes here; 20 ... 24 / 30 ... 34 = the TV-L1 /
                       // TV-KL solves and reverse sweeps, 41 ... 47 / 51 ... 57 = their tangent sweeps, in the weighted sweep's planes;
                       // MODEL_SRUN: the tape as well, variant 0 = taped solve, 1 = reverse sweep;
                       // MODEL_COLOR: the tape as well (nullptr: none), variant 10 * channels + 0 = taped solve, + 1 = reverse sweep,
                       // + 2 = the solve without a tape, + 4 ... 6 = its tangent sweep, by the tangents it reads, its planes here;
                       // 100 + 10 * channels + 0 / 2 / 3 / 4 = the weighted form's taped solve, plain solve and reverse sweep
                       // without / with grad_w)
    const void* tab;   // step table (one per (maxiter, steps, L, dual-first shift, gamma): TabKey)
    int from_state;    // 1: the sequence starts from a prepared state (params.init / order), not from x = f, y = 0
    const void* alpha; // the parameter the launches read: a sweep's blocks and the dataset's parameter are different
                       // buffers, while a float handle's state (f32_state) is the same for both contexts
    int istride;       // doubles between per-image parameter blocks (bpltv_denoise_each, bpltv_sumregs_denoise_each: they live
                       // in d_alpha like a shared parameter, and run other kernel arguments / instances)
    int wo;            // weighted model: weight planes (d_w, d_f and the state sets are fixed for the life of the handle)
    int spacing;       // taped solves and reverse sweeps: checkpoint spacing (0: the full tape).  One sequence holds every
                       // segment of the call, so the segments are part of the graph and a call shape has one graph per chain
    const void* seg;   // checkpointed reverse sweep: its segment tape and recompute planes (bpltv_handle::d_seg)
    int T2;            // ... and the fusion depth of its recompute launches (T: of its reverse launches)
    bool operator<(const GraphKey& o) const {
        return std::tie(maxiter, T, variant, am, an, chains, rho, tau0, sigma0, accel, dbg, nimg, state, tab, from_state, alpha, istride, wo, spacing, seg, T2) <
               std::tie(o.maxiter, o.T, o.variant, o.am, o.an, o.chains, o.rho, o.tau0, o.sigma0, o.accel, o.dbg, o.nimg, o.state, o.tab, o.from_state, o.alpha, o.istride, o.wo,
                        o.spacing, o.seg, o.T2);
    }
};

// Bounded cache of instantiated launch sequences, one hipGraphExec_t per launch chain.  A full cache is emptied.
struct GraphCache {
    size_t bound = 8;
    std::map<GraphKey, std::vector<hipGraphExec_t>> map;
    const std::vector<hipGraphExec_t>* find(const GraphKey& k) const {
        const auto it = map.find(k);
        return it == map.end() ? nullptr : &it->second;
    }
    void make_room() {   // on a miss, before the new sequence is built
        if (map.size() >= bound) drop();
    }
    const std::vector<hipGraphExec_t>* insert(const GraphKey& k, std::vector<hipGraphExec_t> ex) { return &(map[k] = std::move(ex)); }
    void drop() {
        for (auto& kv : map)
            for (auto e : kv.second) (void)hipGraphExecDestroy(e);
        map.clear();
    }
};

struct TabKey {
    int maxiter, accel;
    double tau0, sigma0;
    double L;    // operator-norm estimate the steps are divided by: sqrt(8) (TV), sqrt(18) (sum of regularisers),
                 // or params.opnorm
    int shift;   // 1: row k carries sigma_{k+1} (dual-first order: the dual step of iteration k+1 follows the
                 // primal step of iteration k inside the fused kernel)
    double gamma = 1.0;   // strong convexity of the data term the acceleration uses: 1, or min w of a weighted solve
    bool operator<(const TabKey& o) const {
        return std::tie(maxiter, accel, tau0, sigma0, L, shift, gamma) < std::tie(o.maxiter, o.accel, o.tau0, o.sigma0, o.L, o.shift, o.gamma);
    }
};

}  // namespace

struct MultiState;   // shards, worker threads and the RCCL communicator of a multi-device handle (below)

// The streams of a device, shared by all its handles.  HIP maps streams onto a few hardware queues (four by default) as they
// are created; with a stream pair per handle, the two launch chains of a second handle's solve can land on ONE queue and
// run one after the other -- measured: the 5000-iteration denoise of the reference batch 5.8 -> 11.1 ms on a handle
// created while another one is alive (the reference's workflow: a training set and a validation set), back to 6.0 ms with
// GPU_MAX_HW_QUEUES=8.  So the first handle of a device creates the main stream and the chain streams back to back
// (neighbouring queues), later handles reuse them, the last one to go destroys them.  The library is quiescent when an ABI
// call returns, so handles used one after the other never meet on a stream; handles driven from several host threads at
// once are ordered by the streams they share (each keeps its own events).
struct DeviceStreams {
    hipStream_t main = nullptr;
    std::vector<hipStream_t> chains;
    int refs = 0;
};
static std::mutex g_streams_mu;
static std::map<int, DeviceStreams> g_streams;

static hipError_t device_streams_acquire(int device, hipStream_t* main) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    DeviceStreams& ds = g_streams[device];
    if (ds.refs == 0) {
        hipError_t e = hipStreamCreateWithFlags(&ds.main, hipStreamNonBlocking);
        if (e != hipSuccess) { ds.main = nullptr; return e; }
        hipStream_t cs = nullptr;
        e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);      // the second launch chain, next to the main stream
        if (e != hipSuccess) { (void)hipStreamDestroy(ds.main); ds.main = nullptr; return e; }
        ds.chains.push_back(cs);
    }
    ++ds.refs;
    *main = ds.main;
    return hipSuccess;
}
// chain stream c (0-based) of the device, created on first use
static hipError_t device_streams_chain(int device, size_t c, hipStream_t* out) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    DeviceStreams& ds = g_streams[device];
    while (ds.chains.size() <= c) {
        hipStream_t cs = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        ds.chains.push_back(cs);
    }
    *out = ds.chains[c];
    return hipSuccess;
}
static void device_streams_release(int device) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    auto it = g_streams.find(device);
    if (it == g_streams.end() || it->second.refs <= 0) return;
    if (--it->second.refs == 0) {
        for (auto cs : it->second.chains) (void)hipStreamDestroy(cs);
        if (it->second.main) (void)hipStreamDestroy(it->second.main);
        g_streams.erase(it);
    }
}


// bpltv_set_option (include/bpltv.h): aids for tests and measurements; nothing here changes a result.
struct HandleOptions {
    double adjoint_budget_mb = 0.0;   // > 0: HBM the adjoint's factor workspace may take (forces image groups)
    double sr_sweep_budget_mb = 0.0;  // > 0: HBM the state of a sum-of-regularisers sweep may take (forces parameter groups)
    int sr_force_lu = 0;              // 1: the LU variant of the nested dissection on the symmetric sum-of-regularisers systems too
    int nd_leaf = 0;                  // > 0: leaf size (pixels) of the nested-dissection tree; 0 = 32
    int nd_wave = 1;                  // 0: the workgroup-per-front kernel on every small level (cross-check of nd_front_wave_kernel)
    int nd_skinny = 1;                // 0: fronts of <= 32 pivots through nd_front_small_kernel / the large-regime kernels (cross-check of nd_front_skinny*_kernel)
    int nd_skinny_min = -1, nd_skinny2_min = -1;   // >= 0: (front, image) pairs a level needs for those kernels (-1: the defaults below)
    int nd_staged = 1;                // 0: substitutions of the small levels by the column-loop kernels (cross-check of nd_*_staged_kernel: same bits)
    int hb_sync = 0;                  // HBM band cross-check solver: 0 automatic, 1 HIP events, 2 stream memory operations (fails if unavailable)
    int hb_single_stream = 0;         // ... 1: its three streams folded into one (rocprofv3 --pmc)
    int hb_rw = 0;                    // ... 32 / 128: row width of its trailing update (0 automatic)
    int tape_checkpoint = 0;          // unrolled solves and sweeps: 0 the full tape, C >= 1 a checkpoint every C iterations, -1 automatic
};

// The tape of a taped solve (bpltv_unrolled_denoise and its weighted and sum-of-regularisers forms) that the handle keeps for
// the reverse sweep, with the call that recorded it.  One per model: a tape of one model never stands in for another.
struct Tape {
    double* d = nullptr;
    size_t cap = 0;                 // doubles
    bool valid = false;
    bool each = false;              // recorded by an _each solve: one parameter block per image
    int maxiter = 0, am = 0, an = 0, accel = 0;
    int wo = 0;                     // weighted model: weight planes (0 otherwise)
    double tau0 = 0.0, sigma0 = 0.0, opnorm = 0.0;
    double gamma = 0.0;             // weighted model: min w, the strong convexity its step table was made with
    int spacing = 0;                // 0: the full tape; C >= 1: the buffer holds the state every C iterations (checkpoints) instead
    int channels = 0;               // channel-coupled model: planes of a colour image (0 otherwise)
    // a buffer of `need` doubles when the tape is smaller (*grown; nullptr when it is large enough): allocated ahead of
    // time, so that a call that is rejected afterwards frees it again and leaves the tape as it was
    hipError_t grow(size_t need, double** grown) const {
        *grown = nullptr;
        return cap < need ? hipMalloc((void**)grown, need * sizeof(double)) : hipSuccess;
    }
    void install(double* grown, size_t need) {   // (grown may be nullptr: nothing to do)
        if (!grown) return;
        if (d) (void)hipFree(d);
        d = grown;
        cap = need;
    }
    void record(const bpltv_params& p, int am_, int an_, bool each_, int wo_, double gamma_, int spacing_) {
        valid = true; each = each_; spacing = spacing_;
        maxiter = p.maxiter; am = am_; an = an_; accel = p.accel ? 1 : 0; wo = wo_;
        tau0 = p.tau0; sigma0 = p.sigma0; opnorm = p.opnorm; gamma = gamma_;
    }
    // the call (params, parameter shape, weight planes) is the one that recorded the tape; `each` and `gamma` are compared apart
    bool made_with(const bpltv_params& p, int am_, int an_, int wo_) const {
        return maxiter == p.maxiter && am == am_ && an == an_ && wo == wo_ && accel == (p.accel ? 1 : 0) && tau0 == p.tau0 &&
               sigma0 == p.sigma0 && opnorm == p.opnorm;
    }
    void release() {
        if (d) (void)hipFree(d);
        *this = Tape{};
    }
};

struct bpltv_handle {
    MultiState* multi = nullptr;   // non-null: this handle only fans out to its shards (multi_gpu.hpp)
    int M = 0, N = 0, O = 0, device = 0, ncu = 0;
    size_t npx = 0, tot = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr;   // what the launch chains wait for: everything enqueued on `stream` before the fork
    std::unique_ptr<ShardWorker> launcher;   // persistent host thread that launches the second chain's graph (lazy)
    HandleOptions opt;              // bpltv_set_option: test / measurement aids, all 0 = automatic
    bool has_data = false;
    // dataset + state
    double *d_ubar = nullptr, *d_f = nullptr;
    double* d_state[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    // bpltv_sweep solves its K*O problems in state sets of its own (SolveCtx below)
    double* d_sweep[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    size_t sweep_cap = 0;  // images
    double* d_sweep_cost = nullptr;
    // ... and reads its own K parameter blocks (with the float twin f32_sweep_alpha), so that d_alpha and the last
    // result stay as they were
    double* d_sweep_alpha = nullptr;
    size_t sweep_alpha_cap = 0;
    int result_buf = 0;  // which state set holds the last result
    bool has_result = false;
    bool has_per_image = false;  // d_perimg (cost) and d_red (gradient partials) hold the last evaluate's rows
    double* d_alpha = nullptr;
    size_t alpha_cap = 0;
    int last_am = 1, last_an = 1;
    int alpha_istride = 0;        // 0: d_alpha holds one parameter for every image; am*an (TV) or 3*am*an (sum of
                                  // regularisers): O blocks, one per image (bpltv_denoise_each, bpltv_sumregs_denoise_each),
                                  // which the PDHG and gap kernels of the dataset context address
    double alpha_min = 0.0;       // smallest entry of the last uploaded parameter (validated on the host)
    double* d_partial = nullptr;  // [1 + am*an]
    size_t partial_cap = 0;
    double* d_red = nullptr;      // reduction scratch
    size_t red_cap = 0;
    double* d_perimg = nullptr;   // [O] cost per image / gap per image
    double* d_scalar = nullptr;   // [4]
    std::map<TabKey, double*> tabs;
    // dtype = 32 (opt-in): float twins of everything pdhg_tile_kernel reads and writes; the result is widened into
    // the double state buffers after the solve, so that loss, gap, adjoint and the copies out are the f64 code
    int dtype = 64;
    float* f32_state[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    size_t f32_state_cap = 0;      // images
    float *f32_f = nullptr, *f32_alpha = nullptr, *f32_sweep_alpha = nullptr;
    size_t f32_alpha_cap = 0, f32_sweep_alpha_cap = 0;
    bool f32_f_valid = false;
    std::map<TabKey, float*> tabs32;
    GraphCache graphs[NMODELS] = {{16}, {8}, {8}, {8}, {8}, {8}};   // by Model: at most 16 TV sequences, 8 of each other model
    std::vector<hipStream_t> chain_streams;   // the device's (DeviceStreams), not owned
    std::vector<hipEvent_t> chain_events;
    unsigned* d_phase = nullptr;              // the word chain 0's launches rewrite (PDHG_PHASE_STAMP, pdhg_phase_gate_kernel)
    hipStream_t capture_stream = nullptr;     // the handle's own: stream capture only (nothing ever runs on it); a capture on a shared stream
                                              // would collide with another handle of the device capturing from its own thread
    // adjoint workspace (lazy)
    bool adj_ready = false;   // common workspace
    bool band_ready = false;  // banded Cholesky workspace (LDS window or HBM band)
    bool bcr_ready = false;   // block cyclic reduction workspace
    double* d_bcr = nullptr;  // 7 block arrays [Oc][N][MP*MP]: Linv, LinvT, C, XA, XAT, XB, XBT
    int bcr_MP = 0;
    int bcr_cap = 0;          // images the block arrays hold (the adjoint runs in groups of at most that many)
    NdSolver nd;              // nested-dissection (multifrontal) Cholesky: wide images (nd_solver.hpp)
    NdSolver nd_sr;           // the same for the 13-point stencil of the sum-of-regularisers model
    double* d_coef = nullptr;   // 8 planes
    double* d_band4 = nullptr;  // 4 planes
    double* d_L = nullptr;
    double *d_invF = nullptr, *d_invB = nullptr;  // inverted 64x64 diagonal blocks of L, two layouts (x2 sides)
    double *d_L1 = nullptr, *d_dump = nullptr, *d_Lm = nullptr, *d_spill = nullptr;  // twisted factorisation
    bool adj_twisted = false;
    bool adj_hbm = false;  // M too wide for the LDS window: band factored in place in HBM (hb_band_solver.hpp)
    HbBandSolver hb;
    double *d_p = nullptr, *d_r = nullptr, *d_gpix = nullptr;
    double* d_resn = nullptr;
    int* d_fail = nullptr;
    double *d_u2 = nullptr, *d_ubar2 = nullptr;  // staging for bpltv_gradient (bpltv_vjp: u and the cotangent)
    double* d_gf2 = nullptr;                      // staging of bpltv_vjp's input gradient
    double* d_vjp = nullptr;                      // bpltv_vjp(_device): [4 check words | parameter | parameter gradient]
    size_t vjp_cap = 0;
    double* d_jvp = nullptr;                      // bpltv_jvp's host staging [du | df | dalpha]; bpltv_gauss_newton: [J | e_j | partials | grad, H]
    size_t jvp_cap = 0;
    double* d_jres = nullptr;                     // residual statistics of the directions of a bpltv_jvp with ndir > 1
    size_t jres_cap = 0;
    // sum-of-regularisers model (sumregs_kernels.hpp): state and adjoint workspace, allocated on first use
    double* d_sr[2][7] = {{nullptr}, {nullptr}};   // x, yf1, yf2, yb1, yb2, yc1, yc2; two sets (ping-pong)
    // bpltv_sumregs_sweep solves a group of K_g * O problems in its own state sets, with its own parameter blocks
    double* d_srsweep[2][7] = {{nullptr}, {nullptr}};
    size_t srsweep_cap = 0;                          // problems
    double *d_srsweep_alpha = nullptr, *d_srsweep_cost = nullptr;
    size_t srsweep_alpha_cap = 0, srsweep_cost_cap = 0;
    bool sr_ready = false, sr_adj_ready = false, sr_band_ready = false;
    int last_slices = 1;                            // parameter slices of the last evaluate: 1 (TV) or 3
    int sr_result_buf = 0;
    bool sr_has_result = false;
    bool last_is_sr = false;                        // the last solve was the sum-of-regularisers model
    double *d_srcoef = nullptr, *d_srdiag = nullptr, *d_srw = nullptr, *d_srgpix = nullptr;
    HbBandSolver hb_sr;
    HbLuSolver lu_sr;             // non-symmetric row-scaled system of sumregs_gradient_reg with a patch parameter: banded LU (cross-check)
    NdSolver nd_sr_lu;            // ... the same system by nested dissection (LU variant; the default)
    bool lu_sr_ready = false;
    double* d_srdiagU = nullptr;  // its upper diagonals (7 planes)
    // per-pixel fidelity weight (weighted_kernels.hpp): the handle's copy of the last weighted solve's w (wo planes, gamma =
    // its smallest entry), allocated on first use and never moved; the solve runs in d_state
    double* d_w = nullptr;
    int w_wo = 1;
    double w_min = 0.0;
    bool last_weighted = false;                     // the last solve was bpltv_weighted_denoise: u and the gap are its
    double* d_wst = nullptr;                        // bpltv_weighted_vjp's host staging [f | grad_w], 2 * M*N*O doubles
    // reverse mode through the iterations (tv_tile_kernels.hpp): the handle's own tape of pre-projection duals (allocated on
    // demand, only grows, remembers what it was recorded with), and the reverse sweep's planes [2 sets x (gx, gy1, gy2) | gf | ga | gu]
    Tape tape;
    double* d_unr = nullptr;                        // 9 * M*N*O doubles
    // ... of the weighted model: a tape of its own (z1, z2 and x per iteration), so that a TV
    // tape and a weighted one never stand in for each other, with the weight planes and gamma = min w it was recorded with;
    // the reverse sweep runs in d_unr, its weight gradient in a tenth plane allocated when grad_w is first asked for
    Tape wtape;
    double* d_unr_gw = nullptr;                     // M*N*O doubles
    // ... of the sum-of-regularisers model (sumregs_unrolled_kernels.hpp): a third tape (six dual components per iteration), kept
    // apart from the other two; the reverse sweep runs in planes of its own, [2 sets x (gx, 6 gy) | gf | 3 ga | gu]
    Tape srtape;
    double* d_srunr = nullptr;                      // 19 * M*N*O doubles
    bool srun_ready = false;
    // ... of the channel-coupled model (color_tile_kernels.hpp): a fourth tape, in the TV tape's layout, that remembers the
    // channels it was recorded with; the reverse sweep runs in d_unr.  last_channels: the last solve was this model's, with
    // that many planes per colour image (0: another model's)
    Tape ctape;
    int last_channels = 0;
    // ... and of its weighted form: a fifth tape, in the weighted tape's layout, that remembers the
    // channels, the weight planes and gamma = min w it was recorded with; the reverse sweep runs in d_unr and d_unr_gw
    Tape cwtape;
    // ... of the TV-L1 model: a sixth tape, in the weighted tape's layout, that remembers the weight
    // planes (its gamma is 0 whatever w is); the reverse sweep runs in d_unr and d_unr_gw.  last_l1: the last solve was this model's
    Tape l1tape;
    bool last_l1 = false;
    // ... of the TV-KL model: a seventh tape, as the L1 tape.  last_kl: the last solve was this model's.
    // f_nonneg: the installed dataset is finite and >= 0, as the KL data term needs (-1: not looked at yet, 0: it is not, 1: it
    // is) -- remembered with the dataset, so that it is reduced at most once
    Tape kltape;
    bool last_kl = false;
    int f_nonneg = -1;
    bool color_ready = false;
    bool color_jvp_ready = false;
    // checkpointed reverse sweeps of the four models (option "tape_checkpoint"): [segment tape | 2 recompute state sets],
    // allocated on first use, only grows
    double* d_seg = nullptr;
    size_t seg_cap = 0;                             // doubles
    // forward mode through the iterations (tv_tile_kernels.hpp): the tangent sweep's planes [2 sets x (x, y1, y2, dx, dy1,
    // dy2) | df | dalpha], allocated on first use and never moved
    double* d_ujv = nullptr;                        // 14 * M*N*O doubles
    // ... of the weighted model: planes of its own, [2 sets x 6 | df | dalpha | w | dw] and
    // eight words for the device check of dw, allocated on first use and never moved
    double* d_wjv = nullptr;                        // 16 * M*N*O + 8 doubles
    bool tangent_lds_set[4] = {false, false, false, false};   // TV, weighted, L1, KL: the tangent kernel's dynamic LDS is allowed
    bpltv_stats_t st;
    std::string err;
};

struct MultiState {
    std::vector<bpltv_t*> shard;                         // ordinary single-device handles
    std::vector<int> lo, hi, dev;                        // images [lo, hi) of shard k live on HIP device dev[k]
    std::vector<std::unique_ptr<ShardWorker>> worker;    // one persistent host thread per shard
    std::vector<ncclComm_t> comm;                        // ncclCommInitAll; empty when a device repeats
    int maxloc = 0;                                      // largest shard (rows per rank of the all-gather)
    std::vector<double*> d_rows, d_all;                  // all-gather send / receive buffers per shard
    std::vector<size_t> rows_cap;                        // doubles per row buffer, per shard (a failed allocation on one
                                                         // shard leaves the others' buffers and capacities consistent)
    // Parameter sweeps have a second data-parallel axis (the K parameter blocks): REPLICAS -- one handle per device the
    // caller asked for, each holding ALL O images -- let a dataset with fewer images than devices (the reference's default
    // num_samples = 1, /root/reference/src/BPLDenoising.jl:313; cameraman_128_10 holds one pair) use every device.
    // Created on the first sweep that splits the parameters (multi_sweep), filled from the shards' resident data.
    int dtype = 64;
    std::vector<int> req_dev;                            // every requested device, also those beyond min(nshards, O)
    std::vector<bpltv_t*> rep;                           // replica r lives on req_dev[r]; rep[0] == shard[0] when one shard holds everything
    std::vector<ShardWorker*> rep_worker;                // worker[r] for r < shards, an owned one beyond
    std::vector<std::unique_ptr<ShardWorker>> rep_owned;
    bool rep_data = false;                               // the replicas hold the current dataset
    int sweep_split = 0;                                 // bpltv_set_option "sweep_split": 0 automatic, 1 images, 2 parameters
    bool rep_borrowed0() const { return !rep.empty() && !shard.empty() && rep[0] == shard[0]; }
};

namespace {

int set_err(bpltv_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return set_err(h, BPLTV_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                                  \
    } while (0)

int ensure(bpltv_t* h, double** p, size_t* cap, size_t need) {
    if (*cap >= need) return BPLTV_OK;
    if (*p) HIPCHK(h, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(h, hipMalloc((void**)p, need * sizeof(double)));
    *cap = need;
    return BPLTV_OK;
}

void fill_table(const TabKey& k, std::vector<double>& tab) {
    // oracle/bpltv_oracle.c: bplo_step_table_L (same operations, same order)
    const double L = k.L;
    double tau = k.tau0 / L, sigma = k.sigma0 / L;
    const double gamma = k.gamma;
    tab.assign((size_t)TAB_STRIDE * (k.maxiter > 0 ? k.maxiter : 1), 0.0);
    for (int it = 0; it < k.maxiter; ++it) {
        const double omega = k.accel ? 1.0 / std::sqrt(1.0 + 2.0 * gamma * tau) : 1.0;
        double* r = &tab[(size_t)TAB_STRIDE * it];
        r[0] = tau;
        r[1] = sigma;
        r[2] = omega;
        r[3] = 1.0 / (1.0 + tau);
        r[4] = 1.0 + omega;
        if (k.accel) {
            tau = tau * omega;
            sigma = sigma / omega;
        }
        if (k.shift) r[1] = sigma;   // sigma_{it+1}
    }
}

// operator-norm estimate of a solve: params.opnorm, or the model's bound (sqrt(8) TV, sqrt(18) sum of regularisers)
double opnorm_of(const bpltv_params& p, double L2_default) { return p.opnorm > 0.0 ? p.opnorm : std::sqrt(L2_default); }

int get_table(bpltv_t* h, const bpltv_params& p, double** out, double L2 = 8.0, int shift = 0, double gamma = 1.0) {
    TabKey k{p.maxiter, p.accel ? 1 : 0, p.tau0, p.sigma0, opnorm_of(p, L2), shift, gamma};
    auto it = h->tabs.find(k);
    if (it != h->tabs.end()) {
        *out = it->second;
        return BPLTV_OK;
    }
    std::vector<double> tab;
    fill_table(k, tab);
    double* d = nullptr;
    HIPCHK(h, hipMalloc((void**)&d, tab.size() * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->tabs[k] = d;
    *out = d;
    return BPLTV_OK;
}

// ---- dtype = 32: float twins of the PDHG kernel's operands -------------------------------------------------------
void cvt_to_f32(bpltv_t* h, const double* src, float* dst, size_t n) {
    const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL(cvt_f64_f32_kernel, dim3(nb), dim3(256), 0, h->stream, src, dst, n);
}
void cvt_to_f64(bpltv_t* h, const float* src, double* dst, size_t n) {
    const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL(cvt_f32_f64_kernel, dim3(nb), dim3(256), 0, h->stream, src, dst, n);
}
// Destroy the cached launch sequences of the models in `which` (DROP_* bits).  A graph holds the pointers its kernel
// arguments carried when it was built, so whatever frees or moves one of them drops the graphs that can hold it:
//   d_alpha grows (upload_alpha)                                          every model: all three read it
//   the float twins grow (f32_prepare: f32_state, f32_alpha, f32_sweep_alpha)   TV: only its kernels have a float form
//   the TV sweep's state sets or parameter blocks grow (bpltv_sweep)      TV
//   the sum-of-regularisers sweep's planes or blocks grow (bpltv_sumregs_sweep)   sum of regularisers
// d_f, d_w, the dataset state sets (d_state, d_sr) and the step tables live as long as the handle.
enum { DROP_TV = 1 << MODEL_TV, DROP_SR = 1 << MODEL_SR, DROP_W = 1 << MODEL_W, DROP_UN = 1 << MODEL_UN, DROP_SRUN = 1 << MODEL_SRUN,
       DROP_ALL = DROP_TV | DROP_SR | DROP_W | DROP_UN | DROP_SRUN };
void drop_graphs(bpltv_t* h, int which);
// step table rounded to float (the oracle's bplo_pdhg_f32 rounds the same f64 table)
int get_table32(bpltv_t* h, const bpltv_params& p, float** out) {
    TabKey k{p.maxiter, p.accel ? 1 : 0, p.tau0, p.sigma0, opnorm_of(p, 8.0), 0};
    auto it = h->tabs32.find(k);
    if (it != h->tabs32.end()) {
        *out = it->second;
        return BPLTV_OK;
    }
    std::vector<double> tab;
    fill_table(k, tab);
    std::vector<float> t32(tab.begin(), tab.end());
    float* d = nullptr;
    HIPCHK(h, hipMalloc((void**)&d, t32.size() * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(d, t32.data(), t32.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->tabs32[k] = d;
    *out = d;
    return BPLTV_OK;
}
// What one PDHG solve works on -- a plain value handed to run_pdhg / run_sr_pdhg and everything below them.  Built in two
// kinds of places: dataset_ctx (the O dataset images with the handle's d_alpha) and the two sweeps (K*O problems, or a
// group of them, in the sweep's own state sets with its own parameter blocks).  The solvers say which state set holds the
// result through a return parameter and write nothing of it into the handle: a solve on the dataset context is committed
// by solve_dataset, a sweep commits nothing -- so the last result, d_alpha and the duality gap survive a sweep.
struct SolveCtx {
    double* const* state[2] = {nullptr, nullptr};   // the two state sets (ping-pong): 3 planes each (TV), 7 (sum of regularisers)
    int nimg = 0;                   // problems; problem img reads f[img % O]
    const double* alpha = nullptr;  // the parameter buffer (Float64)
    bool sweep = false;             // float handle: the parameter's twin is f32_sweep_alpha, not f32_alpha (f32_state is shared)
    int astride = 0;                // doubles between the parameter blocks of a sweep (problem img reads block img / O)
    int istride = 0;                // doubles between per-image blocks (bpltv_denoise_each: am*an, bpltv_sumregs_denoise_each:
                                    // 3*am*an; dataset context only)
    int am = 1, an = 1;             // parameter shape
    double alpha_min = 0.0;         // its smallest entry, validated on the host or by alpha_check_kernel
};
SolveCtx dataset_ctx(bpltv_t* h, bool sr) {
    SolveCtx x;
    for (int s = 0; s < 2; ++s) x.state[s] = sr ? h->d_sr[s] : h->d_state[s];
    x.nimg = h->O; x.alpha = h->d_alpha; x.istride = h->alpha_istride;
    x.am = h->last_am; x.an = h->last_an; x.alpha_min = h->alpha_min;
    return x;
}

// buffers for the solve context (x.nimg images) and fresh float copies of f and of the parameter
int f32_prepare(bpltv_t* h, const SolveCtx& x) {
    if (h->f32_state_cap < (size_t)x.nimg) {
        drop_graphs(h, DROP_TV);   // graph nodes hold the old pointers
        for (int s = 0; s < 2; ++s)
            for (int c = 0; c < 3; ++c) {
                if (h->f32_state[s][c]) HIPCHK(h, hipFree(h->f32_state[s][c]));
                h->f32_state[s][c] = nullptr;
                HIPCHK(h, hipMalloc((void**)&h->f32_state[s][c], (size_t)x.nimg * h->npx * sizeof(float)));
            }
        h->f32_state_cap = (size_t)x.nimg;
    }
    if (!h->f32_f) HIPCHK(h, hipMalloc((void**)&h->f32_f, h->tot * sizeof(float)));
    if (!h->f32_f_valid) {
        cvt_to_f32(h, h->d_f, h->f32_f, h->tot);
        h->f32_f_valid = true;
    }
    // the float twin of the context's parameter: the dataset's, or a sweep's blocks
    float*& a32 = x.sweep ? h->f32_sweep_alpha : h->f32_alpha;
    size_t& cap32 = x.sweep ? h->f32_sweep_alpha_cap : h->f32_alpha_cap;
    const size_t cap = x.sweep ? h->sweep_alpha_cap : h->alpha_cap;
    if (cap32 < cap) {
        drop_graphs(h, DROP_TV);
        if (a32) HIPCHK(h, hipFree(a32));
        a32 = nullptr;
        cap32 = 0;
        HIPCHK(h, hipMalloc((void**)&a32, cap * sizeof(float)));
        cap32 = cap;
    }
    cvt_to_f32(h, x.alpha, a32, cap);
    HIPCHK(h, hipGetLastError());
    return BPLTV_OK;
}
// operand pointers of the PDHG kernel for this handle's dtype (float arrays travel in PdhgArgs' double* fields)
inline double* pdhg_state(bpltv_t* h, const SolveCtx& x, int set, int c) {
    return h->dtype == 32 ? reinterpret_cast<double*>(h->f32_state[set][c]) : x.state[set][c];
}
inline const double* pdhg_f(bpltv_t* h) { return h->dtype == 32 ? reinterpret_cast<const double*>(h->f32_f) : h->d_f; }
inline const double* pdhg_alpha(bpltv_t* h, const SolveCtx& x) {
    if (h->dtype == 32) return reinterpret_cast<const double*>(x.sweep ? h->f32_sweep_alpha : h->f32_alpha);
    return x.alpha;
}
// the solve's result (set `buf`) widened into the double state buffers
int f32_widen(bpltv_t* h, const SolveCtx& x, int buf) {
    for (int c = 0; c < 3; ++c) cvt_to_f64(h, h->f32_state[buf][c], x.state[buf][c], (size_t)x.nimg * h->npx);
    HIPCHK(h, hipGetLastError());
    return BPLTV_OK;
}

void drop_graphs(bpltv_t* h, int which) {
    for (int m = 0; m < NMODELS; ++m)
        if (which & (1 << m)) h->graphs[m].drop();
}

int solve_precheck(bpltv_t* h, const bpltv_params& p, double amin, int what);
// what: PRE_TV or PRE_SR (the model), | PRE_GRADIENT for an evaluate (the adjoint follows the solve), | PRE_REG_ARRAY when
// that adjoint is gradient_reg with a patch or map parameter
enum { PRE_TV = 0, PRE_SR = 1, PRE_GRADIENT = 2, PRE_REG_ARRAY = 4 };
inline int pre_gradient(double delta, const bpltv_params& p, int am, int an) {
    const int reg = !(delta > p.delta_t);   // as evaluate_common
    return PRE_GRADIENT | ((reg && !(am == 1 && an == 1)) ? PRE_REG_ARRAY : 0);
}

// The host-side parameter check of every entry point: n entries, finite and >= 0; *amin receives the smallest.  `name`
// is what the message calls the array ("alpha", "sweep: alphas", ...).
// The reference is defined for alpha >= 0 (alpha = 0: u = f); NaN/Inf or a negative ball radius has no
// meaning on this path and would propagate silently through 5000 iterations.
int check_alpha_host(bpltv_t* h, const char* name, const double* a, size_t n, double* amin) {
    *amin = a[0];
    for (size_t e = 0; e < n; ++e) {
        if (!std::isfinite(a[e]) || a[e] < 0.0)
            return set_err(h, BPLTV_E_ARG, "%s[%zu] = %g: parameters must be finite and >= 0", name, e, a[e]);
        if (a[e] < *amin) *amin = a[e];
    }
    return BPLTV_OK;
}

// The checks of arrays that live in HBM, one read-back and one synchronisation for all of them: `par` (n entries, nullable:
// no such check) must be finite and >= 0 (alpha_check_kernel; *pmin receives its smallest entry), every array of `fin`
// (nullable entries are skipped, at most two) must be finite (finite_check_kernel).  chk: 2 + fin.size() words in HBM --
// [0] the smallest entry of `par` (bits), [1] `par` rejected, [2 + j] fin[j] not finite.  *failed: -1 when everything
// passed, else the first job that did not (0: par, 1 + j: fin[j]) -- the caller words the message.  Reads only.
struct DevArray { const double* p; size_t n; const char* name = nullptr; };   // name: what a message calls it ("cotangent gu")
int check_device_arrays(bpltv_t* h, unsigned long long* chk, DevArray par, std::initializer_list<DevArray> fin, double* pmin, int* failed) {
    auto blocks = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)); };
    unsigned long long chk_h[4] = {0, 0, 0, 0};
    const size_t nw = 2 + fin.size();
    HIPCHK(h, hipMemsetAsync(chk, 0xFF, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(chk + 1, 0, (nw - 1) * sizeof(unsigned long long), h->stream));
    if (par.p) hipLaunchKernelGGL(alpha_check_kernel, blocks(par.n), dim3(256), 0, h->stream, par.p, par.n, chk);
    unsigned long long* word = chk + 2;
    for (const DevArray& a : fin) {
        if (a.p) hipLaunchKernelGGL(finite_check_kernel, blocks(a.n), dim3(256), 0, h->stream, a.p, a.n, word);
        ++word;
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(chk_h, chk, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *failed = -1;
    for (size_t j = nw; j-- > 1;)
        if (chk_h[j] != 0) *failed = (int)j - 1;
    if (par.p) std::memcpy(pmin, chk_h, sizeof(double));
    return BPLTV_OK;
}

// The parameter of the dataset context into d_alpha, from the host or (on_device: bpltv_*denoise*_device) from HBM, where
// it is checked in place by alpha_check_kernel (one 16-byte read back) and copied device to device.
// what: the model (PRE_SR: three slices of am*an doubles) and what follows the upload, for solve_precheck.
// blocks: 1, or O for bpltv_denoise_each(_device) and bpltv_sumregs_denoise_each(_device): O blocks of am*an (3*am*an)
// doubles, image k reads block k.
// solve (nullable): the parameters of the PDHG solve the upload is for.  The order is the contract: shape, values,
// solve_precheck, and only then the handle -- a rejected parameter leaves d_alpha, its shape and alpha_min, and so the
// duality gap of the last solve, as they were.
int upload_alpha(bpltv_t* h, const double* alpha, bool on_device, int am, int an, int what = PRE_TV, int blocks = 1,
                 const bpltv_params* solve = nullptr) {
    const bool sr = (what & PRE_SR) != 0;
    if (!alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "alpha: null pointer or empty shape");
    if (am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, sr ? "alpha shape %dx%dx3 exceeds image %dx%d" : "alpha shape %dx%d exceeds image %dx%d",
                       am, an, h->M, h->N);
    const size_t need = (size_t)(sr ? 3 : 1) * blocks * am * an;
    double amin = 0.0;
    if (on_device) {
        int failed = -1;
        if (int rc = check_device_arrays(h, reinterpret_cast<unsigned long long*>(h->d_scalar + 2), {alpha, need}, {}, &amin, &failed)) return rc;
        if (failed == 0) return set_err(h, BPLTV_E_ARG, "alpha (device array): parameters must be finite and >= 0");
    } else if (int rc = check_alpha_host(h, "alpha", alpha, need, &amin)) {
        return rc;
    }
    if (solve)
        if (int rc = solve_precheck(h, *solve, amin, what)) return rc;
    h->alpha_min = amin;
    if (h->alpha_cap < need) {
        drop_graphs(h, DROP_ALL);   // every model's launches read d_alpha
        int rc = ensure(h, &h->d_alpha, &h->alpha_cap, need);
        if (rc) return rc;
    }
    if (h->partial_cap < need + 1) {
        int rc = ensure(h, &h->d_partial, &h->partial_cap, need + 1);
        if (rc) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_alpha, alpha, need * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    h->last_am = am;
    h->last_an = an;
    h->last_slices = sr ? 3 : 1;
    h->alpha_istride = blocks > 1 ? (sr ? 3 : 1) * am * an : 0;
    return BPLTV_OK;
}

// Region, fusion depth and launch chains of one solve: plan_pdhg (tiling.hpp -- plain C++, fuzzed under the sanitizers
// by tools/plan_host_check.cpp) over the geometry of the variant table above.  nimg: problems of the solve.
int make_plan(bpltv_t* h, const bpltv_params& p, Plan* pl, int nimg) {
    static const std::vector<PlanVariant> geom = [] {
        std::vector<PlanVariant> g;
        for (const Variant& V : kVariants) g.push_back(PlanVariant{V.RI, V.RJ, V.tiles_per_block, V.min_image, V.tmax});
        return g;
    }();
    PlanRequest q{h->M, h->N, nimg, h->ncu, p.maxiter, p.tile_iters, p.reserved[0], p.reserved[1]};
    const int rc = plan_pdhg(q, geom.data(), (int)geom.size(), pl);
    switch (rc) {
        case PLAN_OK:
            // pdhg_tile_kernel keeps a launch's step rows in a static LDS array of PDHG_MAX_T rows (only an image that
            // fits one region can ask for more: a halo otherwise caps T at half a region, 31 at most)
            if (kVariants[pl->variant].func_1d && pl->T > PDHG_MAX_T)
                return set_err(h, BPLTV_E_ARG, "tile_iters = %d: the LDS-tile kernels fuse at most %d iterations per launch", pl->T, PDHG_MAX_T);
            return BPLTV_OK;
        case PLAN_E_VARIANT: return set_err(h, BPLTV_E_ARG, "unknown kernel variant %d", p.reserved[0]);
        case PLAN_E_MIN_IMAGE: {
            const Variant& V = kVariants[p.reserved[0] - 1];
            return set_err(h, BPLTV_E_ARG, "kernel variant %d needs an image of at least %dx%d pixels", p.reserved[0], V.RI, V.RJ);
        }
        case PLAN_E_TILE_ITERS: return set_err(h, BPLTV_E_ARG, "tile_iters must be >= 1");
        case PLAN_E_GRID: return set_err(h, BPLTV_E_UNSUPPORTED, "%d problems of %dx%d pixels need more than 2^31 tiles per launch", nimg, h->M, h->N);
        default: return set_err(h, BPLTV_E_ARG, "cannot tile %dx%d with T=%d", h->M, h->N, pl->T);
    }
}

// The words of a launch's arguments that are the same for every workgroup, worked out here instead of by every wave of
// every workgroup, and whether the launch runs the FAST instantiation of pdhg_tile_kernel.  Call with the geometry, the
// parameter's shape, O / Odata, rho, img0 and grid3d set.  FAST indexes with 32 bits: every plane its launches address --
// the state and data planes and a full-map parameter, O * M * N elements at most -- must stay below 2^31 bytes (counted
// with 8-byte elements on float handles too); a larger handle takes the general instantiation, 64-bit indices.
inline void pdhg_fill_invariants(PdhgArgs& a, const Variant& V, int dtype) {
    a.MN = (unsigned long long)a.M * (unsigned long long)a.N;
    a.base0 = a.MN * (unsigned long long)a.img0;
    a.Si = V.RI - 2 * a.halo;
    a.Sj = V.RJ - 2 * a.halo;
    a.amode = (a.am == 1 && a.an == 1) ? 0 : ((a.am == a.M && a.an == a.N) ? 2 : 1);
    a.sweep = (a.O != a.Odata) ? 1 : 0;
    const bool rho0 = dtype == 32 ? ((float)a.rho == 0.0f) : (a.rho == 0.0);   // the test the kernel makes
    const bool narrow = a.MN * (unsigned long long)std::max(a.O, a.Odata) * 8ull < (1ull << 31);
    a.fast = (&V == &kVariants[PLAN_V_TILE32] && a.grid3d && !a.sweep && rho0 && a.amode != 1 && narrow) ? 1 : 0;
#ifdef BPLTV_EXPERIMENTS
    if (a.dbg & 262144) a.fast = 0;   // tools/prologue_ab.py: the general instantiation on the headline solve
#endif
}

// Build one hipGraph per chain (image group): maxiter iterations as a linear launch sequence.
// The chains are replayed concurrently, each on its own stream (= its own hardware queue).
int build_graphs(bpltv_t* h, const SolveCtx& x, const bpltv_params& p, const Plan& pl, const double* d_tab, int niter,
                 bool from_state, std::vector<hipGraphExec_t>* out) {
    const Variant& V = kVariants[pl.variant];
    const int tilesPerImg = pl.nTi * pl.nTj;
    int rc = BPLTV_OK;
    for (int c = 0; c < pl.chains && rc == BPLTV_OK; ++c) {
        const int lo = (int)(((long)x.nimg * c) / pl.chains), hi = (int)(((long)x.nimg * (c + 1)) / pl.chains);
        if (hi <= lo) continue;
        hipGraph_t g = nullptr;
        HIPCHK(h, hipGraphCreate(&g, 0));
        hipGraphNode_t prev = nullptr;
        int cur = from_state ? 1 : 0;   // a prepared start lives in set 1; launch 0 always writes set 0
        // Odd chains run half a launch out of phase: their first launch fuses T/2 iterations only, so that one chain's
        // launch gaps fall into the other chain's arithmetic instead of both idling and both computing together (chains
        // of equal size otherwise stay in lockstep).  Such a chain has one launch more; it starts by writing set 1, so
        // that every chain ends in the same set.  Results do not depend on how the iterations are cut into launches.
        const int h0 = pl.T / 2;
        const bool stagger = (c & 1) && chain_out_of_phase(niter, pl.T, from_state);
        int step = stagger ? h0 : pl.T;
        // two chains: chain 0 stamps its launches, chain 1 falls in at the middle of chain 0's period after its 8th launch,
        // (pdhg_phase_gate_kernel; not in a serial replay's graphs, reserved[2] & 1: a timing aid)
        // (LDS-tile kernels only: launches of ~10 us; the row kernels' launches of ~100 us showed one kind of step only;
        // and launches of at most two workgroups per CU: longer ones -- sweeps of many problems -- are not launch-bound)
        const bool phased = pl.chains == 2 && h->d_phase != nullptr && !(p.reserved[2] & 1) && niter / pl.T >= 64 && V.RI <= 48 &&
                            (long)tilesPerImg * x.nimg <= 4L * (h->ncu > 0 ? h->ncu : 256);
        int nlaunch = 0;
        for (int it = 0; it < niter; it += step, step = pl.T) {
            if (phased && c == 1 && (nlaunch == 8 || nlaunch == 40 || nlaunch == 160)) {   // 40, 160: a check, in case the sequence fell back
                unsigned* ph = h->d_phase;
                int check = nlaunch == 8 ? 0 : 1;
                void* gargs[] = {(void*)&ph, (void*)&check};
                hipKernelNodeParams gp;
                std::memset(&gp, 0, sizeof(gp));
                gp.func = reinterpret_cast<void*>(&pdhg_phase_gate_kernel);
                gp.gridDim = dim3(1); gp.blockDim = dim3(64); gp.sharedMemBytes = 0; gp.kernelParams = gargs; gp.extra = nullptr;
                hipGraphNode_t gate = nullptr;
                if (hipGraphAddKernelNode(&gate, g, prev ? &prev : nullptr, prev ? 1 : 0, &gp) == hipSuccess) prev = gate;
                else (void)hipGetLastError();
            }
            ++nlaunch;
            PdhgArgs a;
            a.f = pdhg_f(h); a.alpha = pdhg_alpha(h, x); a.tab = d_tab; a.rho = p.rho;
            a.am = x.am; a.an = x.an;
            a.M = h->M; a.N = h->N; a.O = x.nimg;
            a.Odata = h->O; a.astride = x.astride; a.istride = x.istride;
            a.nTi = pl.nTi; a.nTj = pl.nTj; a.halo = pl.T; a.seg = V.RJ;
            a.img0 = lo;
            a.phase = (phased && c == 0) ? h->d_phase : nullptr;
#ifdef BPLTV_EXPERIMENTS
            a.dbg = p.reserved[3];
            a.dbg_row[0] = p.tau0; a.dbg_row[1] = p.sigma0; a.dbg_row[2] = 1.0; a.dbg_row[3] = 1.0 / (1.0 + p.tau0); a.dbg_row[4] = 2.0;
#endif
            const int nxt = (it == 0) ? (stagger ? 1 : 0) : 1 - cur;
            a.first = (it == 0 && !from_state) ? 1 : 0;
            // (a first launch takes x = f, y = 0 and ignores what it reads; the FAST instantiation issues the loads all the
            //  same, from the set the launch does not write)
            const int rd = a.first ? 1 - nxt : cur;
            a.xin = pdhg_state(h, x, rd, 0); a.y1in = pdhg_state(h, x, rd, 1); a.y2in = pdhg_state(h, x, rd, 2);
            a.xout = pdhg_state(h, x, nxt, 0); a.y1out = pdhg_state(h, x, nxt, 1); a.y2out = pdhg_state(h, x, nxt, 2);
            a.it0 = it;
            a.nit = std::min(step, niter - it);
            void* kargs[] = {&a};
            hipKernelNodeParams kp;
            std::memset(&kp, 0, sizeof(kp));
            a.ntiles = tilesPerImg * (hi - lo);
            a.xcd = (p.reserved[2] & 2) ? 1 : 0;
            a.grid3d = a.xcd ? 0 : pdhg_grid3d_ok(pl.nTj, hi - lo, V.tiles_per_block);
            pdhg_fill_invariants(a, V, h->dtype);
            kp.func = const_cast<void*>(pdhg_func(V, h->dtype, a.grid3d, a.fast));
            kp.gridDim = a.grid3d ? pdhg_grid(a, a.ntiles) : dim3((tilesPerImg * (hi - lo) + V.tiles_per_block - 1) / V.tiles_per_block);
            kp.blockDim = dim3(V.threads);
            kp.sharedMemBytes = (unsigned)(h->dtype == 32 ? V.lds32 : V.lds);
            kp.kernelParams = kargs;
            kp.extra = nullptr;
            hipGraphNode_t node = nullptr;
            hipError_t e = hipGraphAddKernelNode(&node, g, prev ? &prev : nullptr, prev ? 1 : 0, &kp);
            if (e != hipSuccess) {
                rc = set_err(h, BPLTV_E_HIP, "hipGraphAddKernelNode: %s", hipGetErrorString(e));
                break;
            }
            prev = node;
            cur = nxt;
        }
        if (rc == BPLTV_OK) {
            hipGraphExec_t ex = nullptr;
            hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
            if (e != hipSuccess) rc = set_err(h, BPLTV_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
            else out->push_back(ex);
        }
        (void)hipGraphDestroy(g);
    }
    if (rc != BPLTV_OK) {
        for (auto e : *out) (void)hipGraphExecDestroy(e);
        out->clear();
    }
    return rc;
}

// Launch the TV iterations [it0, it1) of the images [lo, hi) on stream st, from the state set `cur` (ignored when it0 == 0
// and the sequence starts from x = f, y = 0); returns the set holding the result.  stagger: the first launch fuses T/2
// iterations and writes set 1 (an out-of-phase chain, build_graphs).  The signature is the one run_chains asks of every
// model; TV's graphs come from build_graphs, so the driver only calls this with (lo, hi, stagger) = (0, nimg, false) -- the
// eager path and the check_every chunks -- and the image-range and stagger branches below are not taken today.
int enqueue_pdhg(bpltv_t* h, const SolveCtx& x, const bpltv_params& p, const Plan& pl, const double* d_tab, bool from_state,
                 hipStream_t st, int it0, int it1, int cur, int lo, int hi, bool stagger) {
    const Variant& V = kVariants[pl.variant];
    PdhgArgs a;
    a.f = pdhg_f(h);
    a.alpha = pdhg_alpha(h, x);
    a.tab = d_tab;
    a.rho = p.rho;
    a.am = x.am;
    a.an = x.an;
    a.M = h->M; a.N = h->N; a.O = x.nimg;
    a.Odata = h->O; a.astride = x.astride; a.istride = x.istride;
    a.nTi = pl.nTi; a.nTj = pl.nTj; a.halo = pl.T; a.seg = V.RJ;
    a.img0 = lo;
    a.ntiles = pl.nTi * pl.nTj * (hi - lo);
    a.xcd = (p.reserved[2] & 2) ? 1 : 0;
    a.grid3d = a.xcd ? 0 : pdhg_grid3d_ok(pl.nTj, hi - lo, V.tiles_per_block);
#ifdef BPLTV_EXPERIMENTS
    a.dbg = p.reserved[3];
    a.dbg_row[0] = p.tau0; a.dbg_row[1] = p.sigma0; a.dbg_row[2] = 1.0; a.dbg_row[3] = 1.0 / (1.0 + p.tau0); a.dbg_row[4] = 2.0;
#endif
    pdhg_fill_invariants(a, V, h->dtype);
    int step = stagger ? pl.T / 2 : pl.T;
    for (int it = it0; it < it1; it += step, step = pl.T) {
        const int nxt = (it == 0) ? (stagger ? 1 : 0) : 1 - cur;
        a.first = (it == 0 && !from_state) ? 1 : 0;
        const int rd = a.first ? 1 - nxt : cur;   // as build_graphs
        a.xin = pdhg_state(h, x, rd, 0); a.y1in = pdhg_state(h, x, rd, 1); a.y2in = pdhg_state(h, x, rd, 2);
        a.xout = pdhg_state(h, x, nxt, 0); a.y1out = pdhg_state(h, x, nxt, 1); a.y2out = pdhg_state(h, x, nxt, 2);
        a.it0 = it;
        a.nit = std::min(step, it1 - it);
        (h->dtype == 32 ? V.launch32 : V.launch)(a, a.ntiles, st);
        cur = nxt;
    }
    return cur;
}

// Duality gap per image of the iterate in state set `buf` of the dataset context x (the gap kernels address the O dataset
// images only, which is why the sweeps switch check_every off).  MODEL_SR: the three-dual model, seven state planes;
// MODEL_W: the handle's weight d_w, every entry > 0 (the dual objective divides by w: the caller checks w_min).
int compute_gap(bpltv_t* h, const SolveCtx& x, Model model, int buf, double* gap_host /*O or null*/, double* gap_max_host) {
    h->has_per_image = false;   // d_perimg is about to hold the gaps
    const int nblk = 8;
    int rc = ensure(h, &h->d_red, &h->red_cap, (size_t)h->O * nblk * 4);
    if (rc) return rc;
    double* const* S = x.state[buf];
    if (model == MODEL_SR) {
        SrState Ss;
        for (int c = 0; c < 7; ++c) Ss.pl[c] = S[c];
        hipLaunchKernelGGL(sr_gap_partial_kernel, dim3(nblk, h->O), dim3(256), 0, h->stream, Ss, h->d_f, x.alpha, x.am, x.an, h->M,
                           h->N, x.istride, h->d_red);
    } else if (model == MODEL_W) {
        hipLaunchKernelGGL(weighted_gap_partial_kernel, dim3(nblk, h->O), dim3(256), 0, h->stream, S[0], S[1], S[2], h->d_f, h->d_w,
                           h->w_wo > 1 ? h->npx : (size_t)0, x.alpha, x.am, x.an, h->M, h->N, h->d_red);
    } else {
        hipLaunchKernelGGL(gap_partial_kernel, dim3(nblk, h->O), dim3(256), 0, h->stream, S[0], S[1], S[2], h->d_f, x.alpha, x.am,
                           x.an, h->M, h->N, x.istride, h->d_red);
    }
    auto final_kernel = model == MODEL_W ? &weighted_gap_final_kernel : &gap_final_kernel;
    hipLaunchKernelGGL(final_kernel, dim3(1), dim3(256), 0, h->stream, h->d_red, nblk, h->O, h->d_perimg, h->d_scalar);
    HIPCHK(h, hipGetLastError());
    if (gap_host)
        HIPCHK(h, hipMemcpyAsync(gap_host, h->d_perimg, sizeof(double) * h->O, hipMemcpyDeviceToHost, h->stream));
    if (gap_max_host)
        HIPCHK(h, hipMemcpyAsync(gap_max_host, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BPLTV_OK;
}

// Replay the launch chains of one solve: chain 0 on the handle's stream, chain c on chain_streams[c - 1], all forked
// behind what the handle's stream holds now and joined back into it.  threaded: chain 1 is launched from the handle's
// persistent launcher thread (worth it from ~128 launches; short sequences are launched from this thread).  Every
// chain that was started is joined before an error is reported, so nothing is left running behind a failed call.
int launch_chains(bpltv_t* h, const std::vector<hipGraphExec_t>& ex, bool threaded) {
    while (h->chain_streams.size() + 1 < ex.size()) {   // chain 0 runs on the handle's own stream
        hipStream_t cs = nullptr;
        hipEvent_t ce = nullptr;
        HIPCHK(h, device_streams_chain(h->device, h->chain_streams.size(), &cs));   // shared by the handles of the device
        if (hipEventCreateWithFlags(&ce, hipEventDisableTiming) != hipSuccess)
            return set_err(h, BPLTV_E_HIP, "hipEventCreateWithFlags failed (launch chains)");
        h->chain_streams.push_back(cs);
        h->chain_events.push_back(ce);
    }
    HIPCHK(h, hipEventRecord(h->fork_ev, h->stream));
    std::vector<hipError_t> cerr(ex.size(), hipSuccess);
    std::vector<char> started(ex.size(), 0);
    h->st.launch_host_ms[0] = h->st.launch_host_ms[1] = 0.0;
    auto launch_chain = [&](size_t c) {
        hipError_t e = hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        if (c == 0) {
            e = hipGraphLaunch(ex[0], h->stream);
        } else {
            hipStream_t cs = h->chain_streams[c - 1];
            e = hipStreamWaitEvent(cs, h->fork_ev, 0);
            if (e == hipSuccess) { started[c] = 1; e = hipGraphLaunch(ex[c], cs); }
            if (e == hipSuccess) e = hipEventRecord(h->chain_events[c - 1], cs);
        }
        if (c < 2) h->st.launch_host_ms[c] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        cerr[c] = e;
    };
    bool posted = false;
    if (threaded && ex.size() >= 2) {
        if (!h->launcher) {
            try { h->launcher.reset(new ShardWorker(h->device)); } catch (...) { h->launcher.reset(); }
        }
        if (h->launcher) {
            h->launcher->post([&launch_chain]() -> int { launch_chain(1); return 0; });
            posted = true;
        }
    }
    launch_chain(0);
    for (size_t c = posted ? 2 : 1; c < ex.size(); ++c) launch_chain(c);
    if (posted) (void)h->launcher->wait();
    // join every chain that got as far as its stream, whatever happened to the others
    hipError_t first = hipSuccess;
    for (size_t c = 0; c < ex.size(); ++c) {
        if (c >= 1 && started[c]) {
            hipError_t e = (cerr[c] == hipSuccess) ? hipStreamWaitEvent(h->stream, h->chain_events[c - 1], 0)
                                                   : hipStreamSynchronize(h->chain_streams[c - 1]);   // a half-launched chain: drain it
            if (cerr[c] == hipSuccess) cerr[c] = e;
        }
        if (cerr[c] != hipSuccess && first == hipSuccess) first = cerr[c];
    }
    if (first != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipGetLastError();
        return set_err(h, BPLTV_E_HIP, "launch chains: %s", hipGetErrorString(first));
    }
    return BPLTV_OK;
}

// ---- the launch driver shared by the three models ------------------------------------------------------------------------
// One solve = niter iterations cut into launches of T, for `nimg` problems in `chains` image groups.  A model plans (region,
// T, chains), prepares its step table and describes the rest in a ChainSolve; run_chains turns that into launches.
using EnqueueFn = std::function<int(hipStream_t st, int it0, int it1, int cur, int lo, int hi, bool stagger)>;
struct ChainSolve {
    Model model = MODEL_TV;
    int nplanes = 3;             // planes of a state set
    double* const* state0 = nullptr;   // state set 0 (maxiter == 0 writes it)
    int nimg = 0, niter = 0, T = 1, chains = 1;
    bool from_state = false;     // TV: the sequence starts from the prepared state in set 1 (`begin` writes it)
    bool x0_zero = false;        // TV, params.init: maxiter == 0 leaves x = 0, not x = f
    bool serial = false;         // replay the chains one after the other on the handle's stream (TV, reserved[2] & 1)
    bool helper_thread = true;   // long sequences launch chain 1 from the handle's launcher thread (launch_chains)
    double bytes_per_px_iter = 0.0;
    int result_set = -1;         // >= 0: `enqueue` ends every chain in this set, whatever niter and T (segmented sequences)
    std::function<int(bool stagger)> chain_launches;   // optional: launches of one chain of such a sequence (statistics)
    GraphKey key{};
    // launch the iterations [it0, it1) of the images [lo, hi) on st from the state set cur; returns the set holding the
    // result.  stagger: the first launch fuses T/2 iterations and writes set 1
    EnqueueFn enqueue;
    // optional: one graph per chain by other means than a stream capture of `enqueue` (TV: build_graphs)
    std::function<int(std::vector<hipGraphExec_t>*)> build;
    // optional: the largest duality gap of the iterate in set buf -- enables params.check_every / gap_tol
    std::function<int(int buf, double* gmax)> gap;
    // optional: what the timed span holds besides the launches -- in front (TV: pdhg_init_kernel), and behind, with the set
    // holding the result and the iterations done, which it may raise (TV: widening of a float result, closing primal step)
    std::function<int()> begin;
    std::function<int(int buf, int* iterations)> end;
};

// The stagger / ping-pong loop of a ChainSolve::enqueue whose launches tile like the weighted kernel (32 x 32 regions, T
// iterations each): `launch` fills the model's argument struct for one launch -- the iterations [it, it + nit) of the images
// [lo, hi) on st, from the state set cur into nxt; first: it == 0 -- and launches its kernel.  (Defined with the taped solves.)
// Checkpointed taped sequences add: tk0, the tape base iteration of the launch's segment, and a
// checkpoint slot (nplanes planes, M*N*O doubles apart) the launch reads its state from / writes it to instead of a state set.
struct LaunchStep {
    hipStream_t st; int it, nit, cur, nxt, first, lo, hi;
    int tk0 = 0;
    const double* ckin = nullptr;
    double* ckout = nullptr;
};
using LaunchFn = std::function<void(const LaunchStep&)>;
EnqueueFn launch_loop(int T, LaunchFn launch);

// One graph per chain by stream capture of j.enqueue on the handle's capture stream.  Odd chains run half a launch out of
// phase when `out_of_phase` (chain_out_of_phase).  All or nothing: on any failure *out stays empty.
void capture_graphs(bpltv_t* h, const ChainSolve& j, bool out_of_phase, std::vector<hipGraphExec_t>* out) {
    for (int c = 0; c < j.chains; ++c) {
        const int lo = (int)(((long)j.nimg * c) / j.chains), hi = (int)(((long)j.nimg * (c + 1)) / j.chains);
        hipGraph_t g = nullptr;
        hipGraphExec_t ex = nullptr;
        if (!h->capture_stream && hipStreamCreateWithFlags(&h->capture_stream, hipStreamNonBlocking) != hipSuccess) { h->capture_stream = nullptr; break; }
        if (hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            (void)j.enqueue(h->capture_stream, 0, j.niter, 0, lo, hi, (c & 1) && out_of_phase);
            if (hipStreamEndCapture(h->capture_stream, &g) == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess)
                out->push_back(ex);
            if (g) (void)hipGraphDestroy(g);
        }
    }
    if ((int)out->size() != j.chains) {
        for (auto e : *out) (void)hipGraphExecDestroy(e);
        out->clear();
    }
}

// Run the solve j: statistics, maxiter == 0, then either the chunks of params.check_every with a gap check after each, or
// the whole sequence -- replayed from the model's graph cache (built on a miss: j.build or capture_graphs; sequences of
// more than 50000 launches and failed or partial builds are launched eagerly), the chains side by side (launch_chains).  The event
// pair ev[0] / ev[1] brackets everything.  *result_buf: the state set that holds the result (written on success only).
int run_chains(bpltv_t* h, const bpltv_params& p, const ChainSolve& j, int* result_buf) {
    h->st.launches = 0; h->st.iterations = 0; h->st.graph_used = 0; h->st.last_gap = -1.0; h->st.launch_chains = 1;
    h->st.launch_host_ms[0] = h->st.launch_host_ms[1] = 0.0;
    h->st.pdhg_ms = 0.0;
    h->st.bytes_per_px_iter = j.bytes_per_px_iter;
    h->st.algorithmic_bytes = 0.0;
    if (p.maxiter == 0) {   // u = x0 = f for every parameter block (x0_zero: 0), y = 0
        for (int c = 0; c < j.nplanes; ++c) {
            if (c == 0 && !j.x0_zero) {
                for (int r = 0; r < j.nimg / h->O; ++r)
                    HIPCHK(h, hipMemcpyAsync(j.state0[0] + (size_t)r * h->tot, h->d_f, h->tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            } else {
                HIPCHK(h, hipMemsetAsync(j.state0[c], 0, (size_t)j.nimg * h->npx * sizeof(double), h->stream));
            }
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *result_buf = 0;
        return BPLTV_OK;
    }
    const int nl = (j.niter + j.T - 1) / j.T;
    int buf = j.from_state ? 1 : 0, launches = 0, iterations = j.niter;
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (j.begin)
        if (int rc = j.begin()) return rc;
    if (p.check_every > 0 && j.gap) {
        int it = 0;
        while (it < j.niter) {
            const int it1 = std::min(j.niter, it + p.check_every);
            buf = j.enqueue(h->stream, it, it1, buf, 0, j.nimg, false);
            HIPCHK(h, hipGetLastError());
            launches += (it1 - it + j.T - 1) / j.T;
            it = it1;
            double gmax = 0.0;
            if (int rc = j.gap(buf, &gmax)) return rc;   // of the set this chunk just wrote
            h->st.last_gap = gmax;
            if (p.gap_tol > 0.0 && gmax <= p.gap_tol) break;
        }
        iterations = it;
    } else if (j.niter > 0) {
        const std::vector<hipGraphExec_t>* ex = nullptr;
        const bool oop = chain_out_of_phase(j.niter, j.T, j.from_state);
        if (p.use_graph) {
            GraphCache& cache = h->graphs[j.model];
            ex = cache.find(j.key);
            if (!ex && nl <= 50000) {
                cache.make_room();
                std::vector<hipGraphExec_t> built;
                const int brc = j.build ? j.build(&built) : (capture_graphs(h, j, oop, &built), (int)BPLTV_OK);
                (void)hipGetLastError();
                if (brc == BPLTV_OK && (int)built.size() == j.chains) {
                    ex = cache.insert(j.key, std::move(built));
                } else {   // a failed or partial build: nothing of it is kept, the sequence is launched eagerly
                    for (auto e : built) (void)hipGraphExecDestroy(e);
                }
            }
        }
        if (ex) {
            if (ex->size() == 1 || j.serial) {
                for (hipGraphExec_t e : *ex) HIPCHK(h, hipGraphLaunch(e, h->stream));
            } else if (int rc = launch_chains(h, *ex, nl >= 128 && j.helper_thread)) {   // short sequences: a helper thread costs more than it hides
                return rc;
            }
            h->st.launch_chains = (int)ex->size();
            h->st.graph_used = 1;
            buf = j.result_set >= 0 ? j.result_set : chain_result_set(j.niter, j.T);
            launches = chain_launches(j.niter, j.T, (int)ex->size(), oop);
            if (j.chain_launches) {
                launches = 0;
                for (size_t c = 0; c < ex->size(); ++c) launches += j.chain_launches((c & 1) && oop);
            }
        } else {
            buf = j.enqueue(h->stream, 0, j.niter, buf, 0, j.nimg, false);
            HIPCHK(h, hipGetLastError());
            launches = j.chain_launches ? j.chain_launches(false) : nl;
        }
    }
    if (j.end)
        if (int rc = j.end(buf, &iterations)) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->st.pdhg_ms = ms;
    h->st.launches = launches;
    h->st.iterations = iterations;
    h->st.algorithmic_bytes = j.bytes_per_px_iter * (double)h->npx * j.nimg * iterations;
    *result_buf = buf;
    return BPLTV_OK;
}

// The TV solve of the context x; *result_buf: the state set of x that holds the result (written on success only).
int run_pdhg(bpltv_t* h, const SolveCtx& x, const bpltv_params& p, int* result_buf) {
    h->has_per_image = false;
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
    if (p.maxiter < 0) return set_err(h, BPLTV_E_ARG, "maxiter < 0");
    if (p.rho != 0.0 && !(x.alpha_min > 0.0))
        return set_err(h, BPLTV_E_ARG, "rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", x.alpha_min);
    Plan pl;
    int rc = make_plan(h, p, &pl, x.nimg);
    if (rc) return rc;
    // params.init / order (the choices of op_denoise_pdps the reference does not pin): the sequence starts from a
    // prepared state (pdhg_init_kernel) instead of x = f, y = 0; dual-first order = the dual step of iteration 0 in
    // that kernel, maxiter - 1 fused iterations on a table whose row k carries sigma_{k+1}, and the closing primal
    // step (pdhg_xstep_kernel).  Checker: bplo_pdhg_opts.
    const bool from_state = (p.init != 0 || p.order != 0);
    const int main_iters = p.maxiter - (p.order ? 1 : 0);
    if (from_state && h->dtype == 32)
        return set_err(h, BPLTV_E_UNSUPPORTED, "params.init / params.order are implemented for dtype = 64 handles");
    double* d_tab = nullptr;
    if (h->dtype == 32) {
        float* t32 = nullptr;
        rc = get_table32(h, p, &t32);
        if (!rc && p.maxiter > 0) rc = f32_prepare(h, x);
        d_tab = reinterpret_cast<double*>(t32);
    } else {
        rc = get_table(h, p, &d_tab, 8.0, p.order ? 1 : 0);
    }
    if (rc) return rc;
    h->st.tile_iters = pl.T;
    h->st.pdhg_variant = pl.variant + 1;
    h->st.tiles = pl.grid;
    h->st.region_i = kVariants[pl.variant].RI;
    h->st.region_j = kVariants[pl.variant].RJ;
    const size_t total = (size_t)x.nimg * h->npx;
    const unsigned gtot = (unsigned)((total + 255) / 256);
    const bool chunked = p.check_every > 0;
    const bool amap = (x.am == h->M && x.an == h->N) && !(h->M == 1 && h->N == 1);
    ChainSolve j;
    j.model = MODEL_TV; j.nplanes = 3; j.state0 = x.state[0];
    j.nimg = x.nimg; j.niter = main_iters; j.T = pl.T; j.chains = pl.chains;
    j.from_state = from_state; j.x0_zero = p.init != 0;
    // reserved[2] = 1: replay the chains one after the other (no kernels in flight together) -- used by bench.py to time an
    // isolated launch, as rocprofv3 sees it; reserved[2] & 8 (timing aid): both chains launched from the calling thread.
    // hipGraphLaunch walks the graph on the calling thread (a few us of host time per kernel node), so the second chain is
    // launched from the handle's launcher thread -- launched one after the other from this thread the second chain starts
    // when the first is half done and nothing overlaps (measured: 6.83e5 it/s against 8.2e5 on the 10 x 128^2 batch).
    j.serial = (p.reserved[2] & 1) != 0; j.helper_thread = !(p.reserved[2] & 8);
    j.bytes_per_px_iter = (amap ? 64.0 : 56.0) * (h->dtype == 32 ? 0.5 : 1.0);
    j.key = GraphKey{main_iters, pl.T, pl.variant, x.am, x.an, pl.chains, p.rho, p.tau0, p.sigma0, p.accel ? 1 : 0,
                     p.reserved[3] | ((p.reserved[2] & 3) << 16), x.nimg, (const void*)pdhg_state(h, x, 0, 0), (const void*)d_tab,
                     from_state ? 1 : 0, (const void*)pdhg_alpha(h, x), x.istride, 0};
    j.enqueue = [&](hipStream_t st, int it0, int it1, int cur, int lo, int hi, bool stagger) {
        return enqueue_pdhg(h, x, p, pl, d_tab, from_state, st, it0, it1, cur, lo, hi, stagger);
    };
    j.build = [&](std::vector<hipGraphExec_t>* out) { return build_graphs(h, x, p, pl, d_tab, main_iters, from_state, out); };
    j.gap = [&](int buf, double* gmax) {
        if (h->dtype == 32)   // the gap kernels read the double state
            if (int wrc = f32_widen(h, x, buf)) return wrc;
        return compute_gap(h, x, MODEL_TV, buf, nullptr, gmax);
    };
    // the chains fork behind what the handle's stream holds when they start: behind pdhg_init_kernel, while ev[0] -- the
    // timing start -- sits in front of it
    if (from_state)
        j.begin = [&]() {
            hipLaunchKernelGGL(pdhg_init_kernel, dim3(gtot), dim3(256), 0, h->stream, h->d_f, x.alpha, x.am, x.an,
                               h->M, h->N, h->O, x.astride, x.istride, total, p.init ? 1 : 0, p.order ? 1 : 0,
                               p.sigma0 / opnorm_of(p, 8.0), p.rho, x.state[1][0], x.state[1][1], x.state[1][2]);
            HIPCHK(h, hipGetLastError());
            return (int)BPLTV_OK;
        };
    j.end = [&](int buf, int* iterations) {
        if (h->dtype == 32 && !chunked)
            if (int wrc = f32_widen(h, x, buf)) return wrc;
        if (p.order && *iterations == main_iters) {   // dual-first: the primal step of the last iteration
            ++*iterations;
            hipLaunchKernelGGL(pdhg_xstep_kernel, dim3(gtot), dim3(256), 0, h->stream, h->d_f, x.state[buf][1], x.state[buf][2],
                               d_tab + (size_t)TAB_STRIDE * (p.maxiter - 1), h->M, h->N, h->O, total, x.state[buf][0]);
            HIPCHK(h, hipGetLastError());
        }
        return (int)BPLTV_OK;
    };
    return run_chains(h, p, j, result_buf);
}

int compute_cost(bpltv_t* h, const double* d_u, const double* d_ubar, double* d_out /*device scalar*/) {
    const int nblk = 16;
    int rc = ensure(h, &h->d_red, &h->red_cap, (size_t)h->O * nblk * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(cost_partial_kernel, dim3(nblk, h->O), dim3(256), 0, h->stream, d_u, d_ubar, (int)h->npx,
                       h->d_red);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, h->stream, h->d_red, nblk, h->O, 0.5, h->d_perimg,
                       d_out);
    HIPCHK(h, hipGetLastError());
    return BPLTV_OK;
}

size_t adj_factor_lds(int M, int NB) {  // ring (bw+NB) x (bw+1) + panel NB x (bw+NB)
    return sizeof(double) * ((size_t)(M + NB) * (M + 1) + (size_t)NB * (M + NB));
}

// hipMalloc a list of buffers; on failure every buffer of the list is freed again and its pointer cleared, so a
// failed workspace allocation leaves nothing behind (a retry starts from scratch).
struct AllocReq { void** p; size_t bytes; };
int alloc_all(bpltv_t* h, std::initializer_list<AllocReq> reqs, const char* what) {
    for (const AllocReq& r : reqs) *r.p = nullptr;
    for (const AllocReq& r : reqs) {
        const hipError_t e = hipMalloc(r.p, r.bytes);
        if (e != hipSuccess) {
            *r.p = nullptr;
            for (const AllocReq& q : reqs)
                if (*q.p) { (void)hipFree(*q.p); *q.p = nullptr; }
            (void)hipGetLastError();
            return set_err(h, e == hipErrorOutOfMemory ? BPLTV_E_NOMEM : BPLTV_E_HIP, "%s: hipMalloc of %.1f MB failed: %s", what, r.bytes / 1e6,
                           hipGetErrorString(e));
        }
    }
    return BPLTV_OK;
}

int adj_alloc(bpltv_t* h) {
    if (h->adj_ready) return BPLTV_OK;
    const size_t tot = h->tot;
    const int rc = alloc_all(h, {{(void**)&h->d_coef, 8 * tot * sizeof(double)},
                                 {(void**)&h->d_band4, 4 * tot * sizeof(double)},
                                 {(void**)&h->d_p, tot * sizeof(double)},
                                 {(void**)&h->d_r, tot * sizeof(double)},
                                 {(void**)&h->d_gpix, tot * sizeof(double)},
                                 {(void**)&h->d_resn, 4 * (size_t)h->O * (1 + RESN_BLK) * sizeof(double)},
                                 {(void**)&h->d_fail, (size_t)h->O * sizeof(int)}}, "adjoint workspace");
    if (rc) return rc;
    h->adj_ready = true;
    return BPLTV_OK;
}

// HBM the factor workspace of the adjoint may take: bpltv_set_option "adjoint_budget_mb" (a test aid: forces the
// gradient to run in image groups), else what is free now plus what this handle already holds for it, minus a 2 GB reserve.
size_t adj_budget(const bpltv_t* h, size_t held) {
    if (h->opt.adjoint_budget_mb > 0.0) return (size_t)(h->opt.adjoint_budget_mb * 1e6);
    size_t freeb = 0, totalb = 0;
    (void)hipMemGetInfo(&freeb, &totalb);
    const size_t reserve = 2ull << 30;
    return freeb + held > reserve ? freeb + held - reserve : 0;
}
// images per group so that `per_image` bytes each fit the budget: all O when they fit, at least one
int adj_group(bpltv_t* h, size_t per_image, size_t held, const char* what, int* Oc) {
    const size_t budget = adj_budget(h, held);
    size_t g = per_image ? budget / per_image : (size_t)h->O;
    if (g < 1)
        return set_err(h, BPLTV_E_NOMEM, "adjoint gradient (%s): the factor workspace of ONE %dx%d image needs %.2f GB of HBM, %.2f GB available",
                       what, h->M, h->N, per_image / 1e9, budget / 1e9);
    *Oc = (int)std::min<size_t>(std::min<size_t>(g, (size_t)h->O), 32768);   // images are a grid dimension of the solver kernels
    return BPLTV_OK;
}

// Block cyclic reduction (adjoint_bcr_kernels.hpp) applies to M <= 128, N >= 2; its seven block arrays
// take 7*N*MP^2 doubles per image (117 MB for 128^2; the odd blocks' slots stay unused because level 0
// runs in operator form).  Workspace for groups of *Oc images.
bool bcr_applicable(const bpltv_t* h) { return h->M <= BS_MP && h->N >= 2; }

int bcr_alloc(bpltv_t* h, int* Oc) {
    const int MP = (h->M + 15) / 16 * 16;
    const size_t per = BcrArrays::doubles(h->M, h->N, 1, MP) * sizeof(double);
    int rc = adj_group(h, per, (size_t)h->bcr_cap * per, "block cyclic reduction", Oc);
    if (rc) return rc;
    if (h->bcr_cap >= *Oc) return BPLTV_OK;
    if (h->d_bcr) (void)hipFree(h->d_bcr);
    h->d_bcr = nullptr; h->bcr_cap = 0; h->bcr_ready = false;
    rc = alloc_all(h, {{(void**)&h->d_bcr, (size_t)*Oc * per}}, "adjoint gradient (block cyclic reduction)");
    if (rc) return rc;
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&bcr_potrf_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)bcr_potrf_lds(BS_MP)));
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&bcr0_schur_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)bcr0_schur_lds(BS_MP)));
    h->bcr_MP = MP;
    h->bcr_cap = *Oc;
    h->bcr_ready = true;
    return BPLTV_OK;
}

// Nested-dissection Cholesky (nd_solver.hpp): tree built once per handle, workspace for groups of *Oc images.
int nd_alloc(bpltv_t* h, NdSolver& nd, const NdStencil& st, const char* what, int* Oc, bool lu = false) {
    if (!nd.built) {
        const int rc = nd.build(h->M, h->N, st, h->opt.nd_leaf, lu);
        if (rc) { const std::string m = nd.err; nd.release(); return set_err(h, rc, "adjoint gradient (%s): %s", what, m.c_str()); }
    }
    const size_t per = nd.bytes_per_image();
    int rc = adj_group(h, per, (size_t)nd.cap * per, what, Oc);
    if (rc) return rc;
    rc = nd.alloc(*Oc, h->stream);
    if (rc) return set_err(h, rc, "adjoint gradient (%s): %s", what, nd.err.c_str());
    nd.wave_fronts = h->opt.nd_wave != 0;
    nd.skinny_fronts = h->opt.nd_skinny != 0;
    nd.skinny_min = h->opt.nd_skinny_min >= 0 ? h->opt.nd_skinny_min : 0;
    nd.skinny2_min = h->opt.nd_skinny2_min >= 0 ? h->opt.nd_skinny2_min : 256;   // 10 x 128^2: its levels of 160 / 80 fronts lose 4 %, 40 x 128^2 (640 / 320) gains
    nd.staged_solve = h->opt.nd_staged != 0;
    return BPLTV_OK;
}

// Workspace of a whole-batch band solver in HBM (HbBandSolver, HbLuSolver) at bandwidth bw, refused while it would leave
// less than 2 GB free.  refusal: the message of that, a format of two %.1f (GB needed, GB free); `what` opens the message of
// a failed allocation.
template <class Solver>
int hbm_band_alloc(bpltv_t* h, Solver& s, int bw, const char* what, const char* refusal) {
    size_t freeb = 0, totalb = 0;
    (void)hipMemGetInfo(&freeb, &totalb);
    const size_t need = s.bytes_needed(bw, (int)h->npx, h->O);
    if (need + (2ull << 30) > freeb) return set_err(h, BPLTV_E_NOMEM, refusal, need / 1e9, freeb / 1e9);
    if constexpr (std::is_same<Solver, HbBandSolver>::value) {
        s.opt_sync = h->opt.hb_sync; s.opt_single_stream = h->opt.hb_single_stream; s.opt_rw = h->opt.hb_rw;
    }
    const int rc = s.alloc(bw, (int)h->npx, h->O, h->stream);
    if (rc) return set_err(h, rc, "%s: %s", what, s.err.c_str());
    return BPLTV_OK;
}

int band_alloc(bpltv_t* h) {
    if (h->band_ready) return BPLTV_OK;
    const size_t tot = h->tot;
    const size_t W = (size_t)h->M + 1;
    h->adj_hbm = adj_factor_lds(h->M, 4) > 160 * 1024;
    int rc = BPLTV_OK;
    if (h->adj_hbm) {
        char refusal[400];
        snprintf(refusal, sizeof(refusal), "adjoint gradient: the band and its inverted diagonal blocks of %d images of %dx%d need %%.1f GB of HBM (%%.1f GB free); the nested-dissection factorisation (the default for this shape) needs a fraction of that and runs in image groups",
                 h->O, h->M, h->N);
        rc = hbm_band_alloc(h, h->hb, h->M, "adjoint gradient (HBM band)", refusal);
        if (rc) return rc;
    }
    if (!h->adj_hbm) {
        const size_t nblk = (h->npx + SB - 1) / SB;
        rc = alloc_all(h, {{(void**)&h->d_L, tot * W * sizeof(double)},
                           {(void**)&h->d_invF, 2 * (size_t)h->O * nblk * SB * SB * sizeof(double)},
                           {(void**)&h->d_invB, 2 * (size_t)h->O * nblk * SB * SB * sizeof(double)}}, "adjoint gradient (LDS band)");
        if (rc) return rc;
    }
    {   // two-sided (twisted) factorisation: two workgroups per image meet in a dense middle block
        const AdjSplit sp = adj_split((int)h->npx, h->M);
        const size_t midb = sizeof(double) * ((size_t)sp.nm * (sp.nm + 1) + sp.nm);
        h->adj_twisted = !h->adj_hbm && sp.m >= ADJ_G && sp.nbot >= ADJ_G && sp.nm <= 140 && midb <= 160 * 1024 &&
                         sp.nm >= h->M && (size_t)sp.nm <= (size_t)h->M + 4;
        if (h->adj_twisted) {
            const size_t blk = (size_t)(h->M + ADJ_G) * (h->M + ADJ_G);
            rc = alloc_all(h, {{(void**)&h->d_L1, tot * W * sizeof(double)},
                               {(void**)&h->d_dump, 2 * (size_t)h->O * blk * sizeof(double)},
                               {(void**)&h->d_Lm, (size_t)h->O * blk * sizeof(double)},
                               {(void**)&h->d_spill, 2 * (size_t)h->O * RING * sizeof(double)}}, "adjoint gradient (LDS band, twisted)");
            if (rc) {
                for (double** q : {&h->d_L, &h->d_invF, &h->d_invB})
                    if (*q) { (void)hipFree(*q); *q = nullptr; }
                return rc;
            }
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&adj_mid_factor_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&adj_mid_solve_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        }
    }
    if (!h->adj_hbm) {
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&adj_factor_kernel<8, 128>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&adj_factor_kernel<8, 0>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&adj_factor_kernel<4, 0>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    h->band_ready = true;
    return BPLTV_OK;
}

// ---- the three factorisations of the reduced adjoint system ----------------------
enum AdjMethod { ADJ_BAND_LDS = 1, ADJ_BCR = 2, ADJ_BAND_HBM = 3, ADJ_BAND_LU = 4, ADJ_ND = 5, ADJ_ND_LU = 6 };   // also bpltv_stats_t::adjoint_method

// Pick the factorisation for this handle (params.reserved[4]: 0 automatic, 1 banded Cholesky, 2 block cyclic
// reduction, 3 nested dissection), make sure its workspace exists and say in groups of how many images the gradient
// runs (*Oc = O unless the factor workspace of all images does not fit: adj_group).
// Automatic = nested dissection for every shape: it needs the fewest flop and the least memory at every size measured
// (10 x 128^2: factor + solve 0.66 + 0.20 ms against 1.0 + 0.16 ms per solve of block cyclic reduction; 8 x 1024^2:
// 31 + 6 ms against 350 + 70 ms of the HBM band).  The other three stay selectable as cross-checks.
int adj_choose(bpltv_t* h, const bpltv_params& p, AdjMethod* out, int* Oc) {
    const int want = p.reserved[4];
    *Oc = h->O;
    if (want == 2) {
        if (!bcr_applicable(h))
            return set_err(h, BPLTV_E_UNSUPPORTED, "block cyclic reduction needs M <= %d and N >= 2 (M = %d, N = %d)", BS_MP,
                           h->M, h->N);
        const int rc = bcr_alloc(h, Oc);
        if (rc == BPLTV_OK) *out = ADJ_BCR;
        return rc;
    }
    if (want == 0 || want == 3) {
        const int rc = nd_alloc(h, h->nd, nd_stencil_tv(), "nested dissection", Oc);
        if (rc == BPLTV_OK) *out = ADJ_ND;
        return rc;
    }
    const int rc = band_alloc(h);   // whole batch at once (the HBM band path keeps its pipeline state per handle)
    if (rc) return rc;
    *out = h->adj_hbm ? ADJ_BAND_HBM : ADJ_BAND_LDS;
    return BPLTV_OK;
}

// Banded Cholesky in HBM (M > 138): hb_band_solver.hpp / adjoint_hbm_kernels.hpp; the matrix is handed over as
// the four diagonals of adj_assemble_kernel.
int factor_band_hbm(bpltv_t* h) {
    BandDiags D;
    D.planes = h->d_band4; D.tot = h->tot; D.nd = 4;
    D.off[0] = 0; D.off[1] = 1; D.off[2] = h->M - 1; D.off[3] = h->M;
    const int rc = h->hb.factor(D, h->d_fail);
    if (rc) return set_err(h, rc, "adjoint gradient (HBM band): %s", h->hb.err.c_str());
    return BPLTV_OK;
}

// vec <- A^-1 vec, accv += solution; d_gpix is free during the solves and holds y.
void solve_band_hbm(bpltv_t* h, double* vec, double* accv) { h->hb.solve(vec, accv, h->d_gpix); }

// Banded Cholesky with the trailing window in LDS (M <= 138), twisted when the shape allows.
struct LdsBandPlan {
    int tw;
    unsigned nblk;
    AdjSplit sp;
    size_t mid_lds;
    double *invF1, *invB1;
    explicit LdsBandPlan(const bpltv_t* h) {
        tw = h->adj_twisted ? 1 : 0;
        nblk = (unsigned)((h->npx + SB - 1) / SB);
        sp = adj_split((int)h->npx, h->M);
        mid_lds = sizeof(double) * ((size_t)sp.nm * (sp.nm + 1) + sp.nm);
        invF1 = h->d_invF + (size_t)h->O * nblk * SB * SB;
        invB1 = h->d_invB + (size_t)h->O * nblk * SB * SB;
    }
};

void factor_band_lds(bpltv_t* h) {
    const int M = h->M, N = h->N, O = h->O;
    const LdsBandPlan pl(h);
    const dim3 fgrid(O, pl.tw ? 2 : 1);
    if (M == 128)  // compile-time instance: addressing folded
        hipLaunchKernelGGL((adj_factor_kernel<8, 128>), fgrid, dim3(ADJ_FT), adj_factor_lds(M, 8), h->stream,
                           h->d_band4, M, N, O, h->d_L, h->d_L1, pl.tw, h->d_dump, h->d_fail);
    else if (adj_factor_lds(M, 8) <= 160 * 1024)
        hipLaunchKernelGGL((adj_factor_kernel<8, 0>), fgrid, dim3(ADJ_FT), adj_factor_lds(M, 8), h->stream,
                           h->d_band4, M, N, O, h->d_L, h->d_L1, pl.tw, h->d_dump, h->d_fail);
    else
        hipLaunchKernelGGL((adj_factor_kernel<4, 0>), fgrid, dim3(ADJ_FT), adj_factor_lds(M, 4), h->stream,
                           h->d_band4, M, N, O, h->d_L, h->d_L1, pl.tw, h->d_dump, h->d_fail);
    if (pl.tw) {
        hipLaunchKernelGGL(adj_mid_factor_kernel, dim3(O), dim3(256), pl.mid_lds, h->stream, h->d_band4, h->d_dump, M, N, O,
                           h->d_Lm, h->d_fail);
        hipLaunchKernelGGL(adj_invdiag_kernel, dim3(pl.nblk, O), dim3(64), 0, h->stream, h->d_L, M, N, pl.sp.m, h->d_invF,
                           h->d_invB);
        hipLaunchKernelGGL(adj_invdiag_kernel, dim3(pl.nblk, O), dim3(64), 0, h->stream, h->d_L1, M, N, pl.sp.nbot, pl.invF1,
                           pl.invB1);
    } else {
        hipLaunchKernelGGL(adj_invdiag_kernel, dim3(pl.nblk, O), dim3(64), 0, h->stream, h->d_L, M, N, (int)h->npx,
                           h->d_invF, h->d_invB);
    }
}

void solve_band_lds(bpltv_t* h, double* vec, double* accv) {
    const int M = h->M, N = h->N, O = h->O;
    const LdsBandPlan pl(h);
    if (pl.tw) {
        hipLaunchKernelGGL(adj_solve_tw_kernel<0>, dim3(O, 2), dim3(256), 0, h->stream, h->d_L, h->d_L1, h->d_invF,
                           h->d_invB, M, N, vec, accv, h->d_spill);
        hipLaunchKernelGGL(adj_mid_solve_kernel, dim3(O), dim3(256), pl.mid_lds, h->stream, h->d_Lm, M, N, vec, accv,
                           h->d_spill);
        hipLaunchKernelGGL(adj_solve_tw_kernel<1>, dim3(O, 2), dim3(256), 0, h->stream, h->d_L, h->d_L1, h->d_invF,
                           h->d_invB, M, N, vec, accv, h->d_spill);
    } else {
        hipLaunchKernelGGL(adj_solve_kernel, dim3(O), dim3(256), 0, h->stream, h->d_L, h->d_invF, h->d_invB, M, N, vec, accv);
    }
}

// What one adjoint solve reads and writes besides u: the parameter (device, am*an doubles, its smallest entry checked
// on the host or by alpha_check_kernel), the source of the right-hand side -- ubar of the loss 0.5||u - ubar||^2, or
// the cotangent gu of a vector-Jacobian product -- and the outputs.  The resident parameter of the last solve
// (d_alpha, last_am / last_an, alpha_min) is read only by the callers that pass it (gradient_ctx).
struct GradCtx {
    const double* alpha = nullptr;
    int am = 1, an = 1;
    int astride = 0;               // 0: one parameter for every image; am*an (3*am*an, sum of regularisers): image k reads block k
                                   // (bpltv_vjp_each, bpltv_sumregs_vjp_each)
    bool each = false;             // d_out receives the O per-image parameter gradients (image-major), not their sum
    double alpha_min = 0.0;
    const double* src = nullptr;   // ubar, or gu when cot
    bool cot = false;
    double* d_out = nullptr;       // am*an parameter gradient (O*am*an when each), or nullptr: no per-pixel terms, no reduction
    double* d_grad_f = nullptr;    // M*N*O input gradient (+-S q), or nullptr
    // forward mode (bpltv_jvp): ndir > 0 tangent directions solved against ONE factorisation per image group; src, cot,
    // d_out and d_grad_f are then unused.  df: ndir * M*N*O doubles or nullptr; dalpha: ndir blocks of am*an doubles
    // (each: of O * am*an, direction then image; sum of regularisers: 3*am*an) or nullptr; du: ndir * M*N*O doubles --
    // all in HBM, direction-major.
    int ndir = 0;
    const double* df = nullptr;
    const double* dalpha = nullptr;
    double* du = nullptr;
    // weighted model (bpltv_weighted_vjp; reg = 0, cot): w != nullptr selects the system diag(w) + K in its node-scaled form
    // (weighted_adj_setup_kernel).  w: wo planes in HBM, every entry > 0; d_grad_f then receives w o p; d_grad_w (wo planes,
    // or nullptr) receives -(u - f) o p, summed over the images in image order when wo == 1; f is read for d_grad_w only.
    const double* w = nullptr;
    int wo = 1;
    double w_min = 0.0;            // smallest entry of w (the reverse sweep of the weighted iterations: gamma of its step table)
    const double* f = nullptr;
    double* d_grad_w = nullptr;
};
GradCtx gradient_ctx(const bpltv_t* h, const double* d_ubar, double* d_out) {
    GradCtx g;
    g.alpha = h->d_alpha; g.am = h->last_am; g.an = h->last_an; g.alpha_min = h->alpha_min;
    g.src = d_ubar; g.d_out = d_out;
    return g;
}

// ---- the adjoint driver shared by the models ---------------------------------------------------------
// One adjoint solve = per image group the coefficient planes, the assembly and the factorisation, then per right-hand side
// a solve, refinement sweeps against the matrix-free operator and the residual statistics; behind the groups the reduction
// of the per-pixel gradients over the images and the input gradient.  A model describes its linear system in an AdjSystem;
// run_adjoint turns that into launches.
struct AdjGroup {                  // one image group, handed to every per-group hook
    int c0 = 0, nimg = 0;          // its first image, its images
    size_t o0 = 0, ctot = 0;       // c0 * npx, nimg * npx
    unsigned gpx = 0;              // blocks of 256 threads over its pixels
    const double* ga = nullptr;    // its first image's parameter block
    double kact = 0.0;             // the active-set weight of this attempt
    double *dp = nullptr, *dr = nullptr;   // its solution and residual (d_p, d_r)
    int* dfail = nullptr;
    // written by AdjSystem::factor, read by the copy of the right-hand side and by adj_resnorm_kernel: the right-hand side,
    // the main diagonal of the assembled matrix, and (nullable) the node scaling and the kappa plane
    const double *rhs = nullptr, *diag = nullptr, *s = nullptr, *kap = nullptr;
};
struct AdjPlan {   // what AdjSystem::prepare decides once the workspace exists
    int Oc;                  // images per group
    int method, hb_sync;     // bpltv_stats_t::adjoint_method, ::hb_sync
    int nref;                // refinement sweeps unless params.refine sets them
    const char* pivot_msg;   // a failed factorisation: %d position, %d image
    double* gpix;            // per-pixel parameter gradients: AdjSystem::slices planes of M*N*O doubles
};
struct AdjSystem {
    int slices = 1;          // parameter slices (1 TV, 3 sum of regularisers)
    double kact = 0.0;       // active-set weight, before params.kappa_cap and the retry's scale
    double gate_skip = 1.0;  // the residual gate leaves out the rows whose diagonal carries gate_skip * weight (reg: none)
    const char* alpha_msg = nullptr;   // reg with a patch / map parameter that holds a zero: %g its smallest entry
    const char* gate_msg = nullptr;    // %.3e residual, %.1e gate (and, if it names them, %.3e weight, %d sweeps)
    std::function<int(AdjPlan*)> prepare;   // workspace and choice of the factorisation
    // coefficient planes, assembly and factorisation of a group (forward mode on an LU path: of A^T)
    std::function<int(AdjGroup&)> factor;
    // forward mode: the right-hand side of one direction from its tangents (either may be nullptr), and its du from G.dp
    std::function<void(const AdjGroup&, const double* df, const double* dalpha)> tangent_rhs;
    std::function<int(const AdjGroup&, double* du)> store_du;
    std::function<void(const AdjGroup&, double* out)> residual;              // out <- rhs - A G.dp
    std::function<int(const AdjGroup&, double* vec, double* acc)> solve;     // vec <- A^-1 vec, acc += the solution
    std::function<void(const AdjGroup&)> gradpix;                            // the group's planes of AdjPlan::gpix from G.dp
    std::function<void()> grad_in;   // behind the groups: the input gradient(s), d_p covering the whole batch
};

// One attempt at the weight sys.kact * kappa_scale.  The images are processed in groups of at most Oc (AdjSystem::prepare):
// a group uses the factor workspace of the previous one; the per-pixel gradients of all images are summed at the end, per
// image and in image order, so the result does not depend on the grouping (bitwise).
// Reference: the per-image loop of /root/reference/src/TVLearningFunctionVec.jl:76-81,168-173 -- sequential, no limit.
int run_adjoint_once(bpltv_t* h, const GradCtx& g, int reg, const bpltv_params& p, double kappa_scale, const AdjSystem& sys) {
    AdjPlan pl{h->O, 0, 0, 0, nullptr, nullptr};
    int rc = sys.prepare(&pl);
    if (rc) return rc;
    const int M = h->M, N = h->N, O = h->O, am = g.am, an = g.an, S = sys.slices;
    const size_t tot = h->tot, npx = h->npx, P = (size_t)am * an;
    const double kcap = p.kappa_cap > 0.0 ? p.kappa_cap : 1e14;
    const double kact = std::min(sys.kact, kcap) * kappa_scale;
    const int nref = p.refine < 0 ? pl.nref : p.refine;
    // forward mode: every direction keeps its own residual statistics (the gate takes the worst)
    const bool tangent = g.ndir > 0;
    const int ndir = tangent ? g.ndir : 1;
    double* resn_fin = h->d_resn;
    if (ndir > 1) {
        rc = ensure(h, &h->d_jres, &h->jres_cap, 4 * (size_t)O * ndir);
        if (rc) return rc;
        resn_fin = h->d_jres;
    }
    const size_t dastride = S * P * (g.each ? O : 1);   // doubles between two directions of g.dalpha
    HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_fail, 0, sizeof(int) * O, h->stream));
    int chunks = 0;
    for (int c0 = 0; c0 < O; c0 += pl.Oc, ++chunks) {
        AdjGroup G;
        G.c0 = c0; G.nimg = std::min(pl.Oc, O - c0);
        G.o0 = (size_t)c0 * npx; G.ctot = (size_t)G.nimg * npx;
        G.gpx = (unsigned)((G.ctot + 255) / 256);
        G.ga = g.alpha + (size_t)c0 * g.astride;
        G.kact = kact;
        G.dp = h->d_p + G.o0; G.dr = h->d_r + G.o0; G.dfail = h->d_fail + c0;
        rc = sys.factor(G);
        if (rc) return rc;
        HIPCHK(h, hipGetLastError());
        for (int d = 0; d < ndir; ++d) {   // one pass, or the tangent directions against this group's factorisation
            if (tangent)
                sys.tangent_rhs(G, g.df ? g.df + (size_t)d * tot + G.o0 : nullptr,
                                g.dalpha ? g.dalpha + (size_t)d * dastride + (size_t)c0 * g.astride : nullptr);
            // solve + iterative refinement against the matrix-free operator
            HIPCHK(h, hipMemcpyAsync(G.dp, G.rhs, G.ctot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            rc = sys.solve(G, G.dp, nullptr);
            if (rc) return rc;
            for (int it = 0; it < nref; ++it) {
                sys.residual(G, G.dr);
                rc = sys.solve(G, G.dr, G.dp);
                if (rc) return rc;
            }
            sys.residual(G, G.dr);
            double* resn_part = h->d_resn + 4 * (size_t)O + 4 * (size_t)c0 * RESN_BLK;
            hipLaunchKernelGGL(adj_resnorm_kernel, dim3(RESN_BLK, G.nimg), dim3(256), 0, h->stream, G.dr, G.rhs, G.diag, (int)npx, resn_part,
                               G.s, reg ? (double)HUGE_VAL : sys.gate_skip * kact, G.kap, M);
            hipLaunchKernelGGL(adj_resnorm_final_kernel, dim3((4 * G.nimg + 63) / 64), dim3(64), 0, h->stream, resn_part, G.nimg,
                               resn_fin + 4 * ((size_t)d * O + c0));
            if (tangent) {
                rc = sys.store_du(G, g.du + (size_t)d * tot + G.o0);
                if (rc) return rc;
            }
        }
        if (g.d_out) sys.gradpix(G);
        HIPCHK(h, hipGetLastError());
    }
    // ... then per parameter, over all images (a vector-Jacobian product may not want the parameter gradient): slice k of
    // the result from plane k of the per-pixel gradients
    const bool amap = am == M && an == N && !(M == 1 && N == 1);
    if (g.d_out && g.each) {   // per image, image-major (block k holds image k's slices): nothing is summed over images
        if (amap && S == 1)
            HIPCHK(h, hipMemcpyAsync(g.d_out, pl.gpix, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        else if (amap)
            hipLaunchKernelGGL(sr_gpix_each_kernel, dim3((unsigned)((3 * tot + 255) / 256)), dim3(256), 0, h->stream, pl.gpix, npx, O,
                               g.d_out);
        else
            for (int k = 0; k < S; ++k)
                hipLaunchKernelGGL(patch_sum_kernel, dim3((unsigned)P, O), dim3(256), 0, h->stream, pl.gpix + k * tot, M, N, O, am, an,
                                   1, (int)(S * P), g.d_out + (size_t)k * P);
    } else if (g.d_out && amap) {   // pixelwise parameter maps: plain sums over the images
        for (int k = 0; k < S; ++k)
            hipLaunchKernelGGL(map_sum_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, pl.gpix + k * tot, npx, O,
                               g.d_out + (size_t)k * npx);
    } else if (g.d_out) {
        rc = ensure(h, &h->d_red, &h->red_cap, S * P * O);
        if (rc) return rc;
        for (int k = 0; k < S; ++k)
            hipLaunchKernelGGL(patch_sum_kernel, dim3((unsigned)P, O), dim3(256), 0, h->stream, pl.gpix + k * tot, M, N, O, am, an, O,
                               1, h->d_red + (size_t)k * P * O);
        hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, h->stream, h->d_red, O, (int)(S * P), 1.0, g.d_out, (double*)nullptr);
    }
    sys.grad_in();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    std::vector<int> fail(O);
    std::vector<double> resn(4 * (size_t)O * ndir);
    HIPCHK(h, hipMemcpyAsync(fail.data(), h->d_fail, sizeof(int) * O, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(resn.data(), resn_fin, sizeof(double) * resn.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    h->st.adjoint_ms = ms;
    h->st.reg_gradient_used = reg;
    h->st.adjoint_method = pl.method;
    h->st.adjoint_chunks = chunks;
    h->st.hb_sync = pl.hb_sync;
    h->st.kappa_used = reg ? 0.0 : kact;
    double worst = 0.0, worst_raw = 0.0;
    for (int k = 0; k < O; ++k)
        if (fail[k] != 0) return set_err(h, BPLTV_E_NUMERIC, pl.pivot_msg, fail[k] - 1, k);
    for (size_t k = 0; k < (size_t)O * ndir; ++k) {   // (direction, image) pairs: the worst of them
        const double* q = &resn[4 * k];
        const double raw = std::sqrt(q[0]) / (q[1] > 0 ? std::sqrt(q[1]) : 1.0);
        const double scl = std::sqrt(q[2]) / (q[3] > 0 ? std::sqrt(q[3]) : 1.0);
        if (!(raw <= worst_raw)) worst_raw = raw;   // NaN-propagating max
        if (!(scl <= worst)) worst = scl;
    }
    h->st.adjoint_residual = worst;
    h->st.adjoint_residual_raw = worst_raw;
    if (!(worst <= BPLTV_RESIDUAL_GATE)) return set_err(h, BPLTV_E_NUMERIC, sys.gate_msg, worst, (double)BPLTV_RESIDUAL_GATE, kact, nref);
    return BPLTV_OK;
}

// The reduced system is SPD, but its active-set weight (up to 1e14) sits 14 digits above the O(1)
// terms; should rounding ever produce a non-positive pivot, retry with a 100x smaller weight
// (1e12 still reproduces the hard-constraint limit to ~1e-5).
int run_adjoint(bpltv_t* h, const GradCtx& g, int reg, const bpltv_params& p, const AdjSystem& sys) {
    const bool patch = !(g.am == 1 && g.an == 1);
    if (reg && patch && !(g.alpha_min > 0.0)) return set_err(h, BPLTV_E_ARG, sys.alpha_msg, g.alpha_min);
    double scale = 1.0;
    int rc = BPLTV_OK;
    h->st.adjoint_attempts = 0;
    for (int attempt = 0; attempt < 3; ++attempt, scale *= 1e-2) {
        rc = run_adjoint_once(h, g, reg, p, scale, sys);
        h->st.adjoint_attempts = attempt + 1;
        if (rc != BPLTV_E_NUMERIC) break;
        if (reg) break;   // gradient_reg has no active-set weight to reduce
    }
    // stats.kappa_used / adjoint_attempts say which system produced the gradient; a retry that succeeded is
    // not an error, so the message of the failed attempt does not stay behind
    if (rc == BPLTV_OK) h->err.clear();
    return rc;
}

// The TV and weighted TV systems: AdjCoef, the four diagonals of adj_assemble_kernel and the factorisations of adj_choose.
int run_gradient(bpltv_t* h, const double* d_u, const GradCtx& g, int reg, const bpltv_params& p) {
    const int M = h->M, N = h->N, O = h->O, am = g.am, an = g.an;
    const size_t tot = h->tot, npx = h->npx;
    const int patch = !(am == 1 && an == 1);
    const dim3 blk(256);
    AdjMethod method = ADJ_ND;
    AdjCoef C{};      // coefficient planes of the group: the whole-batch planes at the group's first image
    BcrArrays bcr{};
    AdjSystem sys;
    sys.kact = 1.0 / (patch ? std::sqrt(2.220446049250313e-16) : 2.220446049250313e-16);   // TVLearningFunctionVec.jl:128 / :245
    sys.alpha_msg = "gradient_reg with a patch / pixel-map parameter symmetrises with sqrt(alpha): every entry must be > 0 (min = %g)";
    sys.gate_msg = "adjoint solve: scaled residual %.3e above the gate %.1e (weight %.3e, %d refinement sweeps)";
    sys.prepare = [&](AdjPlan* pl) -> int {
        int rc = adj_alloc(h);
        if (rc) return rc;
        rc = adj_choose(h, p, &method, &pl->Oc);
        if (rc) return rc;
        // Refinement sweeps: every sweep gains ~2 digits with the 1e14 active-set weight of the scalar gradient and
        // 4-5 digits with the 6.7e7 / 1e8 weights of the patch and regularised gradients, where the second sweep
        // already reaches rounding level (round-1 sweep of the refinement count).
        // The HBM band and nested-dissection paths solve with true triangular factors (only 128 x 128 diagonal blocks
        // are inverted): one sweep already reaches the level the block-cyclic-reduction path needs two for
        // (1024^2: pixel map 3.6e-9 / patch 6e-11 / regularised 1e-16 from the converged value after ONE sweep, scalar
        // 1.4e-9 after two).  The regularised systems (gamma = 1e8 instead of 1/eps) need none: 4e-10 / 1e-9 / 5e-11 from
        // the converged value without a sweep, scaled residual <= 4e-12.
        const bool direct = (method == ADJ_BAND_HBM || method == ADJ_ND);
        // Scalar parameter (the 1e14 weight) on a direct factorisation: FOUR sweeps.  Against the literal system on images with a
        // planted active set (tests/test_gpu_tv_active_set.py: blocks, strips across the separators, a constant image; bound 1e-8
        // max|p| + 1e-6 |ref|), worst |difference| of grad_f / grad_alpha and worst fraction of the bound over the cases:
        //     nested dissection   2 sweeps 1.8e-7 / 2.1e-5 (2.2 of the bound: refused)   3: 2.4e-9 / 2.7e-7 (0.022)   4: 4.3e-11 / 3.5e-9 (< 0.001)
        //     band in HBM         2 sweeps 3.7e-9 / 3.3e-7 (0.047)                       3: 1.5e-11 / 1.3e-9           4: 5.1e-12 / 1.2e-11
        // Three would do for w = 1 (a tenth of the bound is the margin kept), but with a per-pixel weight three leave 5.5e-9 of a bound
        // of 1.7e-8 (0.32; 1 x 12 x 140 with a 2 x 125 flat block, tests/test_gpu_weighted_shapes.py) and four 5.8e-11: one count for
        // both, so that bpltv_weighted_vjp with w = 1 stays bpltv_vjp bit for bit without asking what w holds.  Cost: adjoint_ms of
        // the 10 x 128^2 scalar evaluate 0.94 -> 1.28 ms (1.11 with three; median of 20).
        pl->nref = direct ? (reg ? 0 : (patch ? 1 : 4)) : ((patch || reg) ? 2 : 3);
        pl->method = (int)method;
        pl->hb_sync = (method == ADJ_BAND_HBM) ? (h->hb.value_sync ? 2 : 1) : 0;
        pl->pivot_msg = method == ADJ_BCR ? "adjoint Cholesky: non-positive pivot at block %d of image %d"
                                          : (method == ADJ_ND ? "adjoint Cholesky: non-positive pivot at front %d of image %d"
                                                              : "adjoint Cholesky: non-positive pivot at column %d of image %d");
        pl->gpix = h->d_gpix;
        return BPLTV_OK;
    };
    sys.factor = [&](AdjGroup& G) -> int {
        const size_t o0 = G.o0;
        const int nimg = G.nimg;
        C.t1 = h->d_coef + o0; C.t2 = h->d_coef + tot + o0; C.c = h->d_coef + 2 * tot + o0; C.kap = h->d_coef + 3 * tot + o0;
        C.h1 = h->d_coef + 4 * tot + o0; C.h2 = h->d_coef + 5 * tot + o0; C.s = h->d_coef + 6 * tot + o0; C.rhs = h->d_coef + 7 * tot + o0;
        double* band4 = h->d_band4;   // the four diagonals of the group's matrices, planes of nimg * npx doubles
        G.rhs = C.rhs; G.diag = band4; G.s = C.s; G.kap = g.w ? C.kap : nullptr;
        const bool tangent = g.ndir > 0;
        if (g.w && !tangent)
            hipLaunchKernelGGL(weighted_adj_setup_kernel, dim3(G.gpx), blk, 0, h->stream, d_u + o0, g.src + o0,
                               g.w + (g.wo > 1 ? o0 : 0), g.wo > 1 ? npx : (size_t)0, G.ga, am, an, M, N, nimg, G.kact, C);
        else if (tangent || g.cot)   // forward mode: the coefficient planes alone (adj_tangent_rhs_kernel writes each direction's right-hand side)
            hipLaunchKernelGGL(adj_setup_cot_kernel, dim3(G.gpx), blk, 0, h->stream, d_u + o0, (tangent ? d_u : g.src) + o0, G.ga, am,
                               an, g.astride, M, N, nimg, patch, reg, G.kact, C);
        else
            hipLaunchKernelGGL(adj_setup_kernel, dim3(G.gpx), blk, 0, h->stream, d_u + o0, g.src + o0, G.ga, am, an, g.astride, M,
                               N, nimg, patch, reg, G.kact, C);
        hipLaunchKernelGGL(adj_assemble_kernel, dim3(G.gpx), blk, 0, h->stream, C, M, N, nimg, band4);
        if (method == ADJ_BCR) {
            bcr = BcrArrays::carve(h->d_bcr, M, N, nimg, h->bcr_MP);
            bcr_factor_band4_launch(h->stream, bcr, band4, M, N, nimg, h->bcr_MP, G.dfail);
        } else if (method == ADJ_ND) {
            const int r2 = h->nd.factor(band4, G.ctot, nimg, G.dfail);
            if (r2) return set_err(h, r2, "adjoint gradient (nested dissection): %s", h->nd.err.c_str());
        } else if (method == ADJ_BAND_HBM) {
            return factor_band_hbm(h);
        } else {
            factor_band_lds(h);
        }
        return BPLTV_OK;
    };
    sys.solve = [&](const AdjGroup& G, double* vec, double* accv) -> int {
        if (method == ADJ_BCR) bcr_solve_launch(h->stream, bcr, M, N, G.nimg, h->bcr_MP, vec, accv, h->d_band4);
        else if (method == ADJ_ND) {
            const int r2 = h->nd.solve(vec, accv, G.nimg);
            if (r2) return set_err(h, r2, "adjoint gradient (nested dissection, substitution): %s", h->nd.err.c_str());
        }
        else if (method == ADJ_BAND_HBM) solve_band_hbm(h, vec, accv);
        else solve_band_lds(h, vec, accv);
        return BPLTV_OK;
    };
    sys.tangent_rhs = [&](const AdjGroup& G, const double* df, const double* dalpha) {
        hipLaunchKernelGGL(adj_tangent_rhs_kernel, dim3(G.gpx), blk, 0, h->stream, C, df, dalpha, am, an, g.astride, M, N, G.nimg, patch, reg);
    };
    sys.residual = [&](const AdjGroup& G, double* out) {
        hipLaunchKernelGGL(adj_residual_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, M, N, G.nimg, out);
    };
    sys.store_du = [&](const AdjGroup& G, double* du) -> int {
        hipLaunchKernelGGL(adj_du_kernel, dim3(G.gpx), blk, 0, h->stream, C.s, G.dp, G.ctot, du);
        return BPLTV_OK;
    };
    sys.gradpix = [&](const AdjGroup& G) {
        hipLaunchKernelGGL(adj_gradpix_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, M, N, G.nimg, patch, reg, h->d_gpix + G.o0);
    };
    sys.grad_in = [&]() {   // the s plane covers the whole batch after the group loop
        const dim3 gtot((unsigned)((tot + 255) / 256));
        if (g.w) {   // weighted model: w o p, and -(u - f) o p per pixel (d_r is free behind the group loop)
            double* gw = g.d_grad_w ? (g.wo > 1 ? g.d_grad_w : h->d_r) : nullptr;
            if (g.d_grad_f || gw)
                hipLaunchKernelGGL(weighted_adj_out_kernel, gtot, blk, 0, h->stream, h->d_coef + 6 * tot, h->d_p, g.w,
                                   g.wo > 1 ? npx : (size_t)0, d_u, g.f, npx, tot, g.d_grad_f, gw);
            if (gw && g.wo == 1)
                hipLaunchKernelGGL(map_sum_kernel, dim3((unsigned)((npx + 255) / 256)), blk, 0, h->stream, h->d_r, npx, O, g.d_grad_w);
        } else if (g.d_grad_f)
            hipLaunchKernelGGL(adj_gradf_kernel, gtot, blk, 0, h->stream, h->d_coef + 6 * tot, h->d_p, tot, reg, g.d_grad_f);
    };
    return run_adjoint(h, g, reg, p, sys);
}

int sr_adj_alloc(bpltv_t* h) {
    int rc = adj_alloc(h);   // d_p, d_r, d_gpix, d_resn, d_fail
    if (rc) return rc;
    if (h->sr_adj_ready) return BPLTV_OK;
    const size_t tot = h->tot;
    rc = alloc_all(h, {{(void**)&h->d_srcoef, 19 * tot * sizeof(double)},
                       {(void**)&h->d_srdiag, 7 * tot * sizeof(double)},
                       {(void**)&h->d_srw, 6 * tot * sizeof(double)},
                       {(void**)&h->d_srgpix, 3 * tot * sizeof(double)}}, "sum-of-regularisers adjoint workspace");
    if (rc) return rc;
    h->sr_adj_ready = true;
    return BPLTV_OK;
}

// The 13-point system of the sum-of-regularisers model (SrCoef; parameter: three slices of g.am*g.an; g.astride != 0: one
// such block per image, image k reads block k).  Factorisations: nested dissection (default, separators two pixels wide,
// image groups when the workspace does not fit), the HBM band at bandwidth 2M (params.reserved[4] = 1, whole batch: the
// cross-check of the nested dissection), and -- sumregs_gradient_reg with a patch parameter, whose row-scaled system is
// not symmetric (SumRegsLearningFunction.jl:250) -- the LU variant of the nested dissection (banded LU with
// params.reserved[4] = 1).
// Forward mode (g.ndir > 0, bpltv_sumregs_jvp): the directions solve A^T du = df - sum_k w_k o up(dx_k) against one
// factorisation per image group.  The LU paths factor the transpose by swapping the lower and the upper diagonal planes
// (the main diagonal copied across), also where sr_force_lu puts a symmetric system on them; the refinement takes the
// residual of A^T (sr_adj_flux_colscale_kernel).  The planes w_k live in d_srgpix, which only the reverse mode needs.
int run_sr_gradient(bpltv_t* h, const double* d_u, const GradCtx& g, int reg, const bpltv_params& p) {
    const int M = h->M, N = h->N, am = g.am, an = g.an;
    const size_t tot = h->tot;
    const int patch = !(am == 1 && an == 1);
    const bool rowsc = reg && patch;
    const bool lu = rowsc || h->opt.sr_force_lu == 1;   // option "sr_force_lu": test aid, the LU path on the symmetric systems too
    const bool band = p.reserved[4] == 1;     // the band solvers (Cholesky / LU) instead of nested dissection
    const bool tangent = g.ndir > 0;
    const int bw = std::min(2 * M, (int)h->npx - 1);
    const dim3 blk(256);
    SrCoef C{};   // planes keep the whole-batch stride C.tot; the group starts at its first image
    double *diag = nullptr, *diagU = nullptr, *w = nullptr, *gp = nullptr;
    const double* rowscale = nullptr;
    AdjSystem sys;
    sys.slices = 3;
    sys.kact = 1.0 / 2.220446049250313e-16;   // eps() in the vector AND the patch variant (:319, :389)
    // the gate leaves out the rows that carry the active-set weight: the smallest share an active element adds to a
    // diagonal is the centred operator's (1/2)^2 kappa (forward and backward differences add kappa or more)
    sys.gate_skip = 0.25;
    sys.alpha_msg = "sumregs_gradient_reg with a patch parameter needs every entry > 0 (min = %g)";
    sys.gate_msg = "sum-of-regularisers adjoint solve: scaled residual %.3e above the gate %.1e";
    sys.prepare = [&](AdjPlan* pl) -> int {
        int rc = sr_adj_alloc(h);
        if (rc) return rc;
        if (p.reserved[4] == 2) return set_err(h, BPLTV_E_UNSUPPORTED, "block cyclic reduction applies to the TV model only");
        if (lu && !h->d_srdiagU) {
            rc = alloc_all(h, {{(void**)&h->d_srdiagU, 7 * tot * sizeof(double)}}, "sum-of-regularisers adjoint (upper diagonals)");
            if (rc) return rc;
        }
        if (lu && !band) {
            rc = nd_alloc(h, h->nd_sr_lu, nd_stencil_sr(), "sum of regularisers, nested dissection (LU)", &pl->Oc, true);
        } else if (lu) {
            if (!h->lu_sr_ready)
                rc = hbm_band_alloc(h, h->lu_sr, bw, "sum-of-regularisers adjoint (banded LU)",
                                    "sum-of-regularisers adjoint (banded LU): %.1f GB of HBM needed, %.1f GB free");
            if (!rc) h->lu_sr_ready = true;
        } else if (band) {
            if (!h->sr_band_ready)
                rc = hbm_band_alloc(h, h->hb_sr, bw, "sum-of-regularisers adjoint (HBM band)",
                                    "sum-of-regularisers adjoint (HBM band): %.1f GB of HBM needed, %.1f GB free");
            if (!rc) h->sr_band_ready = true;
        } else {
            rc = nd_alloc(h, h->nd_sr, nd_stencil_sr(), "sum of regularisers, nested dissection", &pl->Oc);
        }
        if (rc) return rc;
        // kappa = 1e14 for every parameter kind here: on images with a real active set two sweeps left the gradients up to 5e2
        // times outside 1e-8 max|p| + 1e-6 |.| and four 1.2 times; five leave 0.06 of it on every factorisation
        pl->nref = reg ? 1 : 5;
        pl->method = lu ? (band ? (int)ADJ_BAND_LU : (int)ADJ_ND_LU) : (band ? (int)ADJ_BAND_HBM : (int)ADJ_ND);
        pl->hb_sync = (band && !lu) ? (h->hb_sr.value_sync ? 2 : 1) : 0;
        pl->pivot_msg = lu ? (band ? "sum-of-regularisers adjoint, banded LU without pivoting: zero, tiny or non-finite pivot at column %d of image %d"
                                   : "sum-of-regularisers adjoint, LU without pivoting: zero, tiny or non-finite pivot at front %d of image %d")
                           : (band ? "sum-of-regularisers adjoint Cholesky: non-positive pivot at column %d of image %d"
                                   : "sum-of-regularisers adjoint Cholesky: non-positive pivot at front %d of image %d");
        pl->gpix = h->d_srgpix;
        return BPLTV_OK;
    };
    sys.factor = [&](AdjGroup& G) -> int {
        const size_t o0 = G.o0;
        const int nimg = G.nimg;
        C.tot = tot;
        C.t1 = h->d_srcoef + o0; C.t2 = h->d_srcoef + 3 * tot + o0; C.c = h->d_srcoef + 6 * tot + o0; C.kap = h->d_srcoef + 9 * tot + o0;
        C.h1 = h->d_srcoef + 12 * tot + o0; C.h2 = h->d_srcoef + 15 * tot + o0; C.rhs = h->d_srcoef + 18 * tot + o0;
        diag = h->d_srdiag + o0; diagU = lu ? h->d_srdiagU + o0 : nullptr; w = h->d_srw + o0; gp = h->d_srgpix + o0;
        rowscale = rowsc ? G.ga : nullptr;
        G.rhs = C.rhs; G.diag = diag;
        if (tangent || g.cot)   // forward mode: the coefficient planes alone (sr_tangent_rhs_kernel writes each direction's right-hand side)
            hipLaunchKernelGGL(sr_adj_setup_cot_kernel, dim3(G.gpx), blk, 0, h->stream, d_u + o0, (tangent ? d_u : g.src) + o0, G.ga, am,
                               an, g.astride, M, N, nimg, patch, reg, G.kact, C);
        else
            hipLaunchKernelGGL(sr_adj_setup_kernel, dim3(G.gpx), blk, 0, h->stream, d_u + o0, g.src + o0, G.ga, am, an, g.astride, M,
                               N, nimg, patch, reg, G.kact, C);
        if (lu) HIPCHK(h, hipMemsetAsync(h->d_srdiagU, 0, 7 * tot * sizeof(double), h->stream));
        hipLaunchKernelGGL(sr_adj_assemble_kernel, dim3(G.gpx), blk, 0, h->stream, C, M, N, nimg, diag, rowscale, am, an, g.astride, diagU);
        BandDiags D;
        D.planes = diag; D.tot = tot; D.nd = 7;
        D.off[0] = 0; D.off[1] = 1; D.off[2] = 2; D.off[3] = M - 1; D.off[4] = M; D.off[5] = M + 1; D.off[6] = 2 * M;
        // forward mode on the LU paths: A^T.  Its lower diagonals are A's upper ones and the other way round; the main
        // diagonal is read from the first argument alone, and the assembly left plane 0 of diagU at zero.
        const double *facL = diag, *facU = diagU;
        if (tangent && lu) {
            HIPCHK(h, hipMemcpyAsync(diagU, diag, G.ctot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            facL = diagU; facU = diag;
        }
        int rc = 0;
        if (lu && !band) {
            rc = h->nd_sr_lu.factor_lu(facL, facU, tot, nimg, G.dfail);
            if (rc) return set_err(h, rc, "sum-of-regularisers adjoint (nested dissection, LU): %s", h->nd_sr_lu.err.c_str());
        } else if (lu) {
            BandDiags DL = D, DU = D;
            DL.planes = facL;
            DU.planes = facU;
            rc = h->lu_sr.factor(DL, DU, G.dfail);
            if (rc) return set_err(h, rc, "sum-of-regularisers adjoint (banded LU): %s", h->lu_sr.err.c_str());
        } else if (band) {
            rc = h->hb_sr.factor(D, G.dfail);
            if (rc) return set_err(h, rc, "sum-of-regularisers adjoint (HBM band): %s", h->hb_sr.err.c_str());
        } else {
            rc = h->nd_sr.factor(diag, tot, nimg, G.dfail);
            if (rc) return set_err(h, rc, "sum-of-regularisers adjoint (nested dissection): %s", h->nd_sr.err.c_str());
        }
        if (tangent) hipLaunchKernelGGL(sr_adj_wplane_kernel, dim3(G.gpx), blk, 0, h->stream, C, M, N, nimg, gp);
        return BPLTV_OK;
    };
    sys.solve = [&](const AdjGroup& G, double* v, double* acc) -> int {
        int r2 = 0;
        if (lu && !band) { if ((r2 = h->nd_sr_lu.solve(v, acc, G.nimg))) return set_err(h, r2, "sum-of-regularisers adjoint (nested dissection, LU, substitution): %s", h->nd_sr_lu.err.c_str()); }
        else if (lu) h->lu_sr.solve(v, acc, h->d_gpix);
        else if (band) h->hb_sr.solve(v, acc, h->d_gpix);
        else if ((r2 = h->nd_sr.solve(v, acc, G.nimg))) return set_err(h, r2, "sum-of-regularisers adjoint (nested dissection, substitution): %s", h->nd_sr.err.c_str());
        return BPLTV_OK;
    };
    sys.tangent_rhs = [&](const AdjGroup& G, const double* df, const double* dalpha) {
        hipLaunchKernelGGL(sr_tangent_rhs_kernel, dim3(G.gpx), blk, 0, h->stream, C, (const double*)gp, df, dalpha, am, an, g.astride, M, N, G.nimg);
    };
    sys.residual = [&](const AdjGroup& G, double* out) {
        const bool colsc = tangent && rowsc;   // of A^T: the parameter scales columns, before G_k
        if (colsc)
            hipLaunchKernelGGL(sr_adj_flux_colscale_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, M, N, G.nimg, w, rowscale, am, an, g.astride);
        else
            hipLaunchKernelGGL(sr_adj_flux_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, M, N, G.nimg, w);
        hipLaunchKernelGGL(sr_adj_residual_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, w, M, N, G.nimg, out,
                           colsc ? (const double*)nullptr : rowscale, am, an, g.astride);
    };
    sys.store_du = [&](const AdjGroup& G, double* du) -> int {   // du is the solution itself: straight into the caller's array
        HIPCHK(h, hipMemcpyAsync(du, G.dp, G.ctot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        return BPLTV_OK;
    };
    sys.gradpix = [&](const AdjGroup& G) {
        hipLaunchKernelGGL(sr_adj_gradpix_kernel, dim3(G.gpx), blk, 0, h->stream, C, G.dp, M, N, G.nimg, patch, reg, gp);
    };
    sys.grad_in = [&]() {
        if (g.d_grad_f)
            hipLaunchKernelGGL(sr_adj_gradf_kernel, dim3((unsigned)((tot + 255) / 256)), blk, 0, h->stream, h->d_p, tot, reg, g.d_grad_f);
    };
    return run_adjoint(h, g, reg, p, sys);
}

// sr: the defaults of the sum-of-regularisers model (bpltv_sumregs_default_params: another delta_t)
bpltv_params resolve(const bpltv_params* p, bool sr = false) {
    bpltv_params q;
    if (p) q = *p; else if (sr) bpltv_sumregs_default_params(&q); else bpltv_default_params(&q);
    return q;
}

// Parameter checks shared by every entry point that takes a bpltv_params.
int check_params(bpltv_t* h, const bpltv_params& p) {
#ifndef BPLTV_EXPERIMENTS
    if (p.reserved[3] != 0)
        return set_err(h, BPLTV_E_ARG, "params.reserved[3] must be 0 (the timing-experiment switches exist in tools/ builds only)");
#endif
    if (!(p.tau0 > 0.0) || !(p.sigma0 > 0.0) || !std::isfinite(p.tau0) || !std::isfinite(p.sigma0))
        return set_err(h, BPLTV_E_ARG, "tau0 and sigma0 must be positive and finite");
    if (!(p.rho >= 0.0) || !std::isfinite(p.rho)) return set_err(h, BPLTV_E_ARG, "rho must be >= 0 and finite");
    if (p.reserved[4] < 0 || p.reserved[4] > 3) return set_err(h, BPLTV_E_ARG, "unknown adjoint factorisation %d", p.reserved[4]);
    if ((p.init != 0 && p.init != 1) || (p.order != 0 && p.order != 1)) return set_err(h, BPLTV_E_ARG, "params.init and params.order must be 0 or 1");
    if (!(p.opnorm >= 0.0) || !std::isfinite(p.opnorm)) return set_err(h, BPLTV_E_ARG, "params.opnorm must be >= 0 and finite (0 = default)");
    return BPLTV_OK;
}

struct WallTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

int check_weight(bpltv_t* h, const char* who, const double* w, bool on_device, size_t n, double* wmin);
int weighted_check_params(bpltv_t* h, const bpltv_params& p, const char* who);

// What bpltv_vjp, bpltv_jvp, bpltv_weighted_vjp and their sum-of-regularisers, _each and _device forms do before the
// adjoint solve, `who` ("vjp", "jvp", "weighted_vjp") in every message: parameter shape, params, the parameter on the host
// (check_alpha_host) or in HBM (alpha_dev), the weighted model's w, and the cotangent / tangent arrays `extra` (at most
// two, HBM, nullable) -- all of it checked before anything of the handle changes, the device arrays with one read-back
// (check_device_arrays).  The parameter is then staged in d_vjp = [4 check words | parameter | parameter gradient | w], so
// that the last solve -- d_alpha with its shape and minimum, d_w, the PDHG state and graphs, and so bpltv_u_device and
// bpltv_duality_gap -- stays as it was.  Fills *p (the resolved params) and the parameter fields of *g.
// slices: 1 TV, 3 sum of regularisers (the parameter is 3*am*an doubles).  each: alpha holds O blocks, image k reads block k.
// w (nullable; wo planes): the weighted model, every entry > 0 (w_pos; >= 0 without: the reverse sweep of the iterations
// divides by nothing); staged behind the parameter gradient.
int stage_param(bpltv_t* h, const char* who, const double* alpha, bool alpha_dev, int am, int an, int slices, bool each, int reg,
                const bpltv_params* pp, const double* w, int wo, std::initializer_list<DevArray> extra, bpltv_params* p, GradCtx* g,
                bool w_pos = true) {
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "%s: parameter shape %dx%d (image %dx%d)", who, am, an, h->M, h->N);
    const bool sr = slices == 3;
    *p = resolve(pp);
    if (int prc = w ? weighted_check_params(h, *p, who) : check_params(h, *p)) return prc;
    if (sr && p->reserved[4] == 2) return set_err(h, BPLTV_E_UNSUPPORTED, "block cyclic reduction applies to the TV model only");
    const size_t P = (size_t)slices * am * an * (each ? h->O : 1), nw = w ? (size_t)wo * h->npx : 0;
    double amin = 0.0, wmin = 0.0;
    if (!alpha_dev)
        if (int crc = check_alpha_host(h, (std::string(who) + ": alpha").c_str(), alpha, P, &amin)) return crc;
    if (w) {
        if (int rc = check_weight(h, who, w, alpha_dev, nw, &wmin)) return rc;
        if (w_pos && !(wmin > 0.0)) return set_err(h, BPLTV_E_ARG, "%s: the adjoint system scales with 1/sqrt(w): every weight must be > 0 (min = %g)", who, wmin);
    }
    int rc = ensure(h, &h->d_vjp, &h->vjp_cap, 4 + 2 * P + nw);
    if (rc) return rc;
    int failed = -1;
    rc = check_device_arrays(h, reinterpret_cast<unsigned long long*>(h->d_vjp), {alpha_dev ? alpha : nullptr, P}, extra, &amin, &failed);
    if (rc) return rc;
    if (failed == 0) return set_err(h, BPLTV_E_ARG, "%s: alpha (device array): parameters must be finite and >= 0", who);
    if (failed > 0) return set_err(h, BPLTV_E_ARG, "%s: the %s must be finite", who, extra.begin()[failed - 1].name);
    if (sr && reg && !(am == 1 && an == 1) && !(amin > 0.0))   // run_adjoint's refusal for this model, before anything changes
        return set_err(h, BPLTV_E_ARG, "sumregs_gradient_reg with a patch parameter needs every entry > 0 (min = %g)", amin);
    const hipMemcpyKind kind = alpha_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    double *d_a = h->d_vjp + 4, *d_wv = h->d_vjp + 4 + 2 * P;
    HIPCHK(h, hipMemcpyAsync(d_a, alpha, P * sizeof(double), kind, h->stream));
    if (w) HIPCHK(h, hipMemcpyAsync(d_wv, w, nw * sizeof(double), kind, h->stream));
    g->alpha = d_a; g->am = am; g->an = an; g->alpha_min = amin;
    g->astride = each ? slices * am * an : 0; g->each = each;
    if (w) { g->w = d_wv; g->wo = wo; g->w_min = wmin; }
    return BPLTV_OK;
}

// Vector-Jacobian product of u = denoise(f, alpha) on a single-device handle: d_u, d_gu and the outputs live in HBM
// (the host form stages them), `alpha` on the host or (alpha_dev) in HBM; checks and staging by stage_param.
// slices: 1 TV (bpltv_vjp), 3 sum of regularisers (bpltv_sumregs_vjp; the parameter is 3*am*an doubles).
// d_grad_alpha: slices*am*an doubles in HBM or nullptr; d_grad_f: M*N*O doubles in HBM or nullptr; not both nullptr.
// each (bpltv_vjp_each, bpltv_sumregs_vjp_each): alpha holds O blocks of slices*am*an doubles, image k reads block k, and
// d_grad_alpha receives the O per-image gradients, image-major.
int vjp_common(bpltv_t* h, const double* d_u, const double* alpha, bool alpha_dev, int am, int an, int reg,
               const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha, int slices = 1,
               bool each = false) {
    if (!d_u || !alpha || !d_gu) return set_err(h, BPLTV_E_ARG, "vjp: null pointer");
    if (!d_grad_f && !d_grad_alpha) return set_err(h, BPLTV_E_ARG, "vjp: both outputs are NULL");
    bpltv_params p;
    GradCtx g;
    if (int rc = stage_param(h, "vjp", alpha, alpha_dev, am, an, slices, each, reg, pp, nullptr, 1, {{d_gu, h->tot, "cotangent gu"}}, &p, &g)) return rc;
    g.src = d_gu; g.cot = true;
    g.d_out = d_grad_alpha; g.d_grad_f = d_grad_f;
    h->has_per_image = false;   // the reduction scratch (d_red) no longer holds the last evaluate's rows
    return slices == 3 ? run_sr_gradient(h, d_u, g, reg ? 1 : 0, p) : run_gradient(h, d_u, g, reg ? 1 : 0, p);
}

// Jacobian-vector product of u = denoise(f, alpha) on a single-device handle: the linear map whose transpose
// vjp_common computes, for ndir directions against one factorisation per image group
// (run_adjoint_once).  d_u, the tangents d_df / d_dalpha (either may be nullptr: a zero tangent) and d_du live in HBM,
// direction-major; `alpha` on the host or (alpha_dev) in HBM.  slices: 1 TV (bpltv_jvp), 3 sum of regularisers
// (bpltv_sumregs_jvp; parameter and tangent blocks are 3*am*an doubles).  Checks and staging by stage_param.
int jvp_common(bpltv_t* h, const double* d_u, const double* alpha, bool alpha_dev, int am, int an, int reg,
               const bpltv_params* pp, int ndir, const double* d_df, const double* d_dalpha, double* d_du, bool each,
               int slices = 1) {
    if (!d_u || !alpha || !d_du) return set_err(h, BPLTV_E_ARG, "jvp: null pointer");
    if (ndir < 1) return set_err(h, BPLTV_E_ARG, "jvp: ndir = %d (at least one direction)", ndir);
    if (!d_df && !d_dalpha) return set_err(h, BPLTV_E_ARG, "jvp: both tangents are NULL");
    const size_t P = (size_t)slices * am * an * (each ? h->O : 1);
    bpltv_params p;
    GradCtx g;
    if (int rc = stage_param(h, "jvp", alpha, alpha_dev, am, an, slices, each, reg, pp, nullptr, 1,
                             {{d_df, (size_t)ndir * h->tot, "tangent df"}, {d_dalpha, (size_t)ndir * P, "tangent dalpha"}}, &p, &g))
        return rc;
    g.ndir = ndir; g.df = d_df; g.dalpha = d_dalpha; g.du = d_du;
    return slices == 3 ? run_sr_gradient(h, d_u, g, reg ? 1 : 0, p) : run_gradient(h, d_u, g, reg ? 1 : 0, p);
}

// ============================================================================================
// Sum-of-regularisers model (sumregs_kernels.hpp; /root/reference/src/SumRegsLearningFunction.jl)
// ============================================================================================
// PDHG kernels of the three-dual model: params.variant 1 = sr_tile_kernel<32,32> (one pixel per thread), 2 =
// sr_strip_kernel<3,48,16> (48 x 48 region, three pixels per thread); 0 = by image size.
struct SrVariant {
    int R, threads;
    size_t lds;
    void (*kernel)(SrArgs);
    void (*sweep_kernel)(SrArgs);   // the same kernel for K * O problems of a parameter sweep (f[img % O], block img / O)
    void (*each_kernel)(SrArgs);    // ... for the O images with one parameter block each (f[img], block img)
};
const SrVariant SR_VARIANTS[] = {
    {32, 32 * 32, sr_lds_bytes(32, 32), &sr_tile_kernel<32, 32>, &sr_tile_kernel<32, 32, SR_SWEEP>, &sr_tile_kernel<32, 32, SR_EACH>},
    {48, 48 * 16, sr_lds_bytes(48, 48), &sr_strip_kernel<3, 48, 16>, &sr_strip_kernel<3, 48, 16, SR_SWEEP>,
     &sr_strip_kernel<3, 48, 16, SR_EACH>},
};
constexpr int SR_NVARIANTS = 2;

// What run_pdhg (what = PRE_TV) or run_sr_pdhg (PRE_SR) would reject in a solve of the dataset context with a parameter
// whose smallest entry is amin; PRE_GRADIENT adds what run_gradient / run_sr_gradient reject on the parameters and the
// shape alone (block cyclic reduction where it does not apply; gradient_reg with a patch or map parameter that has a zero
// entry, PRE_REG_ARRAY).  upload_alpha checks this before it touches the handle, so that a rejected call leaves it --
// d_alpha, its shape and minimum, the last result, and so bpltv_duality_gap -- as it was (the sweeps check the same
// before they change anything).
int solve_precheck(bpltv_t* h, const bpltv_params& p, double amin, int what) {
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
    if (p.maxiter < 0) return set_err(h, BPLTV_E_ARG, "maxiter < 0");
    if (p.rho != 0.0 && !(amin > 0.0))
        return set_err(h, BPLTV_E_ARG, "rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", amin);
    const bool sr = (what & PRE_SR) != 0;
    if (!sr) {
        Plan pl;
        if (int rc = make_plan(h, p, &pl, h->O)) return rc;
        if ((p.init != 0 || p.order != 0) && h->dtype == 32)
            return set_err(h, BPLTV_E_UNSUPPORTED, "params.init / params.order are implemented for dtype = 64 handles");
    } else {
        if (p.init != 0 || p.order != 0)
            return set_err(h, BPLTV_E_UNSUPPORTED, "params.init / params.order are implemented for the TV model only");
        if (p.reserved[0] < 0 || p.reserved[0] > SR_NVARIANTS)
            return set_err(h, BPLTV_E_ARG, "variant %d: the sum-of-regularisers model has 1..%d", p.reserved[0], SR_NVARIANTS);
    }
    if (!(what & PRE_GRADIENT)) return BPLTV_OK;
    if (p.reserved[4] == 2) {
        if (sr) return set_err(h, BPLTV_E_UNSUPPORTED, "block cyclic reduction applies to the TV model only");
        if (!bcr_applicable(h))
            return set_err(h, BPLTV_E_UNSUPPORTED, "block cyclic reduction needs M <= %d and N >= 2 (M = %d, N = %d)", BS_MP,
                           h->M, h->N);
    }
    if ((what & PRE_REG_ARRAY) && !(amin > 0.0))
        return set_err(h, BPLTV_E_ARG, sr ? "sumregs_gradient_reg with a patch parameter needs every entry > 0 (min = %g)"
                                          : "gradient_reg with a patch / pixel-map parameter symmetrises with sqrt(alpha): every entry must be > 0 (min = %g)",
                       amin);
    return BPLTV_OK;
}

int sr_alloc(bpltv_t* h) {
    if (h->sr_ready) return BPLTV_OK;
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 7; ++c) HIPCHK(h, hipMalloc((void**)&h->d_sr[s][c], h->tot * sizeof(double)));
    for (const SrVariant& v : SR_VARIANTS)
        for (auto k : {v.kernel, v.sweep_kernel, v.each_kernel})
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds));
    h->sr_ready = true;
    return BPLTV_OK;
}

// maxiter iterations of the three-dual PDHG, T fused per launch (halo 2T), launched by run_chains, on the solve context
// x: x.nimg problems in the state sets x.state; problem img reads f[img % O] and the parameter block img / O (x.astride
// doubles apart) of x.alpha; with x.istride != 0 (dataset context, bpltv_sumregs_denoise_each) image img reads the block
// img, x.istride doubles apart.  *result_buf: the state set that holds the result (written on success only).
int run_sr_pdhg(bpltv_t* h, const SolveCtx& x, const bpltv_params& p, int* result_buf) {
    h->has_per_image = false;
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
    if (p.maxiter < 0) return set_err(h, BPLTV_E_ARG, "maxiter < 0");
    if (p.rho != 0.0 && !(x.alpha_min > 0.0))
        return set_err(h, BPLTV_E_ARG, "rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", x.alpha_min);
    int rc = sr_alloc(h);
    if (rc) return rc;
    double* d_tab = nullptr;
    if (p.init != 0 || p.order != 0)
        return set_err(h, BPLTV_E_UNSUPPORTED, "params.init / params.order are implemented for the TV model only");
    const int nimg = x.nimg;
    double* const* const* S = x.state;   // the planes exist from sr_alloc on (the dataset context points into the handle)
    const double* d_alpha = x.alpha;
    if (nimg > 65535) return set_err(h, BPLTV_E_UNSUPPORTED, "the sum-of-regularisers solve takes at most 65535 problems per launch (problems are a grid dimension)");
    rc = get_table(h, p, &d_tab, 18.0);   // ||G_f||^2 + ||G_b||^2 + ||G_c||^2 <= 8 + 8 + 2 (sumregs_oracle.c: SR_L)
    if (rc) return rc;
    const int M = h->M, N = h->N;
    if (p.reserved[0] < 0 || p.reserved[0] > SR_NVARIANTS) return set_err(h, BPLTV_E_ARG, "variant %d: the sum-of-regularisers model has 1..%d", p.reserved[0], SR_NVARIANTS);
    int vi = p.reserved[0] - 1;
    if (vi < 0) {
        // Both kernels are VALU-issue bound; the 48 x 48 region recomputes 2.25 x instead of 4 x but holds one
        // workgroup per CU.  Fitted on MI355X with the two launch chains in place (ms per 1000 iterations at T = 4,
        // gpurun_out/r3s, 10 ... 40 images of 128^2, 8 x 200^2, 3 ... 6 x 256^2, 4 x 512^2, 2 x 1024^2): the one-pixel kernel
        // 0.6 + 0.0056 per 32 x 32 tile; the strip kernel 5.0 while every CU holds at most one 48 x 48 workgroup, 9.1 for
        // a second round, then 0.0157 per tile.  The strip kernel takes over from about 40 images of 128^2 or 4 of 256^2.
        const int ncu = h->ncu > 0 ? h->ncu : 256;
        auto tiles = [&](int R) {
            const int Tt = std::max(1, std::min(4, std::min((M <= R) ? 4 : (R - 1) / 4, (N <= R) ? 4 : (R - 1) / 4)));
            return (double)tile_count(M, R, 2 * Tt) * tile_count(N, R, 2 * Tt) * nimg;
        };
        const double t32 = tiles(32), t48 = tiles(48);
        const double c32 = 0.6 + 0.0056 * t32;
        const double c48 = t48 <= ncu ? 5.0 : (t48 <= 2 * ncu ? 9.1 : std::max(9.1, 0.0157 * t48));
        vi = (M <= 32 && N <= 32) ? 0 : (c48 < c32 ? 1 : 0);
    }
    const SrVariant& V = SR_VARIANTS[vi];
    const int SR_R = V.R;
    int T = p.tile_iters > 0 ? p.tile_iters : 4;   // halo 8: core 16 of the 32 x 32, 32 of the 48 x 48 region
    auto maxT = [](int L, int R) { return (L <= R) ? (1 << 20) : (R - 1) / 4; };   // 2 * halo = 4T must leave a core
    T = std::min(T, std::min(maxT(M, SR_R), maxT(N, SR_R)));
    if (T < 1) return set_err(h, BPLTV_E_ARG, "tile_iters must be >= 1");
    const int nTi = tile_count(M, SR_R, 2 * T), nTj = tile_count(N, SR_R, 2 * T);
    if (nTi < 1 || nTj < 1) return set_err(h, BPLTV_E_ARG, "cannot tile %dx%d with T=%d", M, N, T);
    const int grid = nTi * nTj * nimg;
    h->st.tile_iters = T; h->st.tiles = grid; h->st.region_i = SR_R; h->st.region_j = SR_R; h->st.pdhg_variant = vi + 1;
    const bool each = x.istride != 0;   // one block per image: the dataset context only (nimg == O)
    void (*kern)(SrArgs) = each ? V.each_kernel : (nimg == h->O ? V.kernel : V.sweep_kernel);
    const bool amap = (x.am == M && x.an == N) && !(M == 1 && N == 1);
    ChainSolve j;
    j.model = MODEL_SR; j.nplanes = 7; j.state0 = S[0];
    j.nimg = nimg; j.niter = p.maxiter; j.T = T;
    j.chains = plan_chains(p.reserved[1], grid, h->ncu, nimg, 2);   // at most two: chain 0 on the handle's stream, chain 1 on a second one
    j.bytes_per_px_iter = amap ? 144.0 : 120.0;   // read x, 6 y, f (+ 3 alpha), write x, 6 y
    j.key = GraphKey{p.maxiter, T, vi, x.am, x.an, j.chains, p.rho, p.tau0, p.sigma0, p.accel ? 1 : 0, 0, nimg, (const void*)S[0][0],
                     (const void*)d_tab, 0, (const void*)d_alpha, x.istride, 0};
    j.enqueue = [&](hipStream_t st, int it0, int it1, int cur, int lo, int hi, bool stagger) {
        int step = stagger ? T / 2 : T;
        for (int it = it0; it < it1; it += step, step = T) {
            SrArgs a;
            const int nxt = (it == 0) ? (stagger ? 1 : 0) : 1 - cur;
            for (int c = 0; c < 7; ++c) { a.in[c] = S[cur][c]; a.out[c] = S[nxt][c]; }
            a.f = h->d_f; a.alpha = d_alpha; a.tab = d_tab; a.rho = p.rho;
            a.am = x.am; a.an = x.an;
            a.it0 = it; a.nit = std::min(step, it1 - it);
            a.M = M; a.N = N; a.O = nimg; a.nTi = nTi; a.nTj = nTj; a.halo = 2 * T;
            a.first = (it == 0) ? 1 : 0;
            a.img0 = lo;
            a.Odata = h->O; a.astride = each ? x.istride : x.astride;
            hipLaunchKernelGGL(kern, dim3(nTi, nTj, hi - lo), dim3(V.threads), V.lds, st, a);
            cur = nxt;
        }
        return cur;
    };
    // duality-gap checks every check_every iterations, early stop at gap_tol (as the TV model)
    j.gap = [&](int buf, double* gmax) { return compute_gap(h, x, MODEL_SR, buf, nullptr, gmax); };
    return run_chains(h, p, j, result_buf);
}

// One solve of the dataset context (TV, or sr: sum of regularisers).  The result is committed to the handle here, after
// the solve succeeded -- the only place where result_buf / has_result / last_is_sr and their sr_ twins are written.
int solve_dataset(bpltv_t* h, bool sr, const bpltv_params& p) {
    int buf = 0;
    const SolveCtx x = dataset_ctx(h, sr);
    const int rc = sr ? run_sr_pdhg(h, x, p, &buf) : run_pdhg(h, x, p, &buf);
    if (rc) return rc;
    (sr ? h->sr_result_buf : h->result_buf) = buf;
    (sr ? h->sr_has_result : h->has_result) = true;
    h->last_is_sr = sr;
    h->last_weighted = false;
    h->last_channels = 0;
    h->last_l1 = false;
    h->last_kl = false;
    return BPLTV_OK;
}
// u of the last solve of the model
inline const double* result_u(const bpltv_t* h, bool sr) { return sr ? h->d_sr[h->sr_result_buf][0] : h->d_state[h->result_buf][0]; }

// The six bpltv_*denoise* entry points on a single-device handle: the parameter from the host or (alpha_dev) from HBM,
// blocks = 1 or O (bpltv_denoise_each), u copied to the host when u_out is given.
int denoise_common(bpltv_t* h, bool sr, const double* alpha, bool alpha_dev, int am, int an, int blocks, const bpltv_params* pp,
                   double* u_out) {
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const bpltv_params p = resolve(pp, sr);
    if (int prc = check_params(h, p)) return prc;
    int rc = upload_alpha(h, alpha, alpha_dev, am, an, sr ? PRE_SR : PRE_TV, blocks, &p);
    if (rc) return rc;
    rc = solve_dataset(h, sr, p);
    if (rc) return rc;
    if (u_out) {
        HIPCHK(h, hipMemcpyAsync(u_out, result_u(h, sr), h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// tv_op_learning_function (TVLearningFunctionVec.jl:14-27) and, sr, sumregs_learning_function (SumRegsLearningFunction.jl:
// 8-36) on a single-device handle.  partial: [cost, grad (slices*am*an)...], to HBM (d_partial_user, TV only) and / or the host.
int evaluate_common(bpltv_t* h, bool sr, const double* alpha, int am, int an, double delta, const bpltv_params* pp,
                    double* u_out, double* d_partial_user, double* partial_host) {
    if (!h) return BPLTV_E_ARG;
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const bpltv_params p = resolve(pp, sr);
    if (int prc = check_params(h, p)) return prc;
    int rc = upload_alpha(h, alpha, false, am, an, (sr ? PRE_SR : PRE_TV) | pre_gradient(delta, p, am, an), 1, &p);
    if (rc) return rc;
    if (!sr && h->band_ready && h->adj_hbm && p.reserved[4] == 1) {   // HBM band path: zero the band while the PDHG solve runs
        const int prc = h->hb.prefill_async();
        if (prc) return set_err(h, prc, "adjoint gradient (HBM band): %s", h->hb.err.c_str());
    }
    rc = solve_dataset(h, sr, p);
    if (rc) return rc;
    const double* d_u = result_u(h, sr);
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
    rc = compute_cost(h, d_u, h->d_ubar, h->d_partial);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev[5], h->stream));
    const int reg = !(delta > p.delta_t);  // TVLearningFunctionVec.jl:21-25; SumRegsLearningFunction.jl:14-18, 30-34
    const GradCtx g = gradient_ctx(h, h->d_ubar, h->d_partial + 1);
    rc = sr ? run_sr_gradient(h, d_u, g, reg, p) : run_gradient(h, d_u, g, reg, p);
    if (rc) return rc;
    const size_t np = 1 + (size_t)(sr ? 3 : 1) * am * an;
    if (d_partial_user)
        HIPCHK(h, hipMemcpyAsync(d_partial_user, h->d_partial, np * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (partial_host)
        HIPCHK(h, hipMemcpyAsync(partial_host, h->d_partial, np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (u_out)
        HIPCHK(h, hipMemcpyAsync(u_out, d_u, h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[4], h->ev[5]));
    h->st.cost_ms = ms;
    h->st.total_ms = wt.ms();
    h->has_per_image = !(am == h->M && an == h->N && !(h->M == 1 && h->N == 1));
    return BPLTV_OK;
}

// ============================================================================================
// Multi-device handle (multi_gpu.hpp): every entry point fans out to the shards' worker threads.
// ============================================================================================
#define NCCLCHK(h, call)                                                                            \
    do {                                                                                            \
        ncclResult_t r_ = (call);                                                                   \
        if (r_ != ncclSuccess)                                                                      \
            return set_err(h, BPLTV_E_HIP, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_),   \
                           __FILE__, __LINE__);                                                     \
    } while (0)

// Run f(k, shard k) on every shard's worker thread and wait for all of them.
template <class F>
int multi_run(bpltv_t* h, F f) {
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    for (int k = 0; k < n; ++k) ms.worker[k]->post([&f, &ms, k]() -> int { return f(k, ms.shard[k]); });
    int rc = BPLTV_OK, bad = -1;
    for (int k = 0; k < n; ++k) {
        const int r = ms.worker[k]->wait();
        if (r != BPLTV_OK && rc == BPLTV_OK) { rc = r; bad = k; }
    }
    if (rc != BPLTV_OK)
        set_err(h, rc, "shard %d (images %d..%d, device %d): %s", bad, ms.lo[bad], ms.hi[bad] - 1, ms.dev[bad],
                ms.shard[bad] ? ms.shard[bad]->err.c_str() : "creation failed");
    return rc;
}

void multi_free(bpltv_t* h) {
    MultiState* ms = h->multi;
    if (!ms) return;
    const int n = (int)ms->shard.size();
    if (!ms->worker.empty()) {
        (void)multi_run(h, [ms](int k, bpltv_t* c) -> int {
            if (k < (int)ms->d_rows.size() && ms->d_rows[k]) (void)hipFree(ms->d_rows[k]);
            if (k < (int)ms->d_all.size() && ms->d_all[k]) (void)hipFree(ms->d_all[k]);
            if (c) (void)bpltv_destroy(c);
            return BPLTV_OK;
        });
    }
    for (size_t r = 0; r < ms->rep.size(); ++r) {   // replicas (not the borrowed shard 0), each on its device's thread
        if (!ms->rep[r] || (r == 0 && ms->rep_borrowed0())) continue;
        bpltv_t* c = ms->rep[r];
        ms->rep_worker[r]->post([c]() -> int { (void)bpltv_destroy(c); return 0; });
        (void)ms->rep_worker[r]->wait();
    }
    ms->rep.clear();
    ms->rep_owned.clear();
    for (ncclComm_t c : ms->comm) (void)ncclCommDestroy(c);
    ms->worker.clear();   // joins the threads
    (void)n;
    delete ms;
    h->multi = nullptr;
}

int multi_create(bpltv_t** out, int M, int N, int O, const int* devices, int nshards, int dtype) {
    if (!out) return BPLTV_E_ARG;
    *out = nullptr;
    if (M < 1 || N < 1 || O < 1 || (dtype != 64 && dtype != 32) || !devices || nshards < 1) return BPLTV_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BPLTV_E_HIP;
    for (int k = 0; k < nshards; ++k)
        if (devices[k] < 0 || devices[k] >= ndev) return BPLTV_E_ARG;
    bpltv_t* h = new (std::nothrow) bpltv_handle();
    if (!h) return BPLTV_E_NOMEM;
    *out = h;   // returned even on failure so that bpltv_last_error works; caller destroys
    h->M = M; h->N = N; h->O = O; h->device = devices[0];
    h->npx = (size_t)M * N;
    h->tot = h->npx * O;
    std::memset(&h->st, 0, sizeof(h->st));
    h->st.M = M; h->st.N = N; h->st.O = O; h->st.device = devices[0];
    h->st.last_gap = -1.0;
    MultiState* ms = new (std::nothrow) MultiState();
    if (!ms) return set_err(h, BPLTV_E_NOMEM, "out of host memory");
    h->multi = ms;
    ms->dtype = dtype;
    ms->req_dev.assign(devices, devices + nshards);
    const int n = std::min(nshards, O);   // no empty image shards; parameter sweeps use the other devices too (replicas)
    std::set<int> distinct;
    for (int k = 0; k < n; ++k) {
        int lo, hi;
        shard_range(O, n, k, &lo, &hi);
        ms->lo.push_back(lo); ms->hi.push_back(hi); ms->dev.push_back(devices[k]);
        ms->maxloc = std::max(ms->maxloc, hi - lo);
        distinct.insert(devices[k]);
        ms->shard.push_back(nullptr);
        ms->worker.emplace_back(new ShardWorker(devices[k]));
    }
    ms->d_rows.assign(n, nullptr);
    ms->d_all.assign(n, nullptr);
    ms->rows_cap.assign(n, 0);
    h->st.ngpus = (int)distinct.size();
    h->st.shards = n;
    int rc = multi_run(h, [ms, M, N, dtype](int k, bpltv_t*) -> int {
        return bpltv_create(&ms->shard[k], M, N, ms->hi[k] - ms->lo[k], ms->dev[k], dtype);
    });
    if (rc) return rc;
    if ((int)distinct.size() == n) {   // one rank per device: RCCL communicator of this process
        ms->comm.assign(n, nullptr);
        ncclResult_t r = ncclCommInitAll(ms->comm.data(), n, ms->dev.data());
        if (r != ncclSuccess) {
            ms->comm.clear();
            return set_err(h, BPLTV_E_HIP, "ncclCommInitAll over %d devices failed: %s", n, ncclGetErrorString(r));
        }
        int cnt = 0;   // what RCCL itself reports for the communicator (bench.py / the tests print it)
        if (ncclCommCount(ms->comm[0], &cnt) == ncclSuccess) h->st.nccl_ranks = cnt;
    }
    return BPLTV_OK;
}

int multi_stats(bpltv_t* h) {   // aggregate the shards' statistics into h->st
    MultiState& ms = *h->multi;
    bpltv_stats_t a = ms.shard[0]->st;
    a.O = h->O; a.device = ms.dev[0];
    for (size_t k = 1; k < ms.shard.size(); ++k) {
        const bpltv_stats_t& b = ms.shard[k]->st;
        a.tiles += b.tiles;
        a.launches = std::max(a.launches, b.launches);
        a.pdhg_ms = std::max(a.pdhg_ms, b.pdhg_ms);
        a.cost_ms = std::max(a.cost_ms, b.cost_ms);
        a.adjoint_ms = std::max(a.adjoint_ms, b.adjoint_ms);
        a.algorithmic_bytes += b.algorithmic_bytes;
        a.last_gap = std::max(a.last_gap, b.last_gap);
        a.adjoint_residual = std::max(a.adjoint_residual, b.adjoint_residual);
        a.adjoint_residual_raw = std::max(a.adjoint_residual_raw, b.adjoint_residual_raw);
        a.kappa_used = std::min(a.kappa_used, b.kappa_used);
        a.adjoint_attempts = std::max(a.adjoint_attempts, b.adjoint_attempts);
        a.iterations = std::max(a.iterations, b.iterations);
    }
    a.ngpus = h->st.ngpus; a.shards = h->st.shards; a.nccl_ranks = h->st.nccl_ranks;
    a.collective = h->st.collective; a.collective_ms = h->st.collective_ms;
    a.total_ms = h->st.total_ms;
    h->st = a;
    return BPLTV_OK;
}

// Run f(r, replica r) on the worker thread of replica r's device, r < cnt, and wait for all of them.
template <class F>
int rep_run(bpltv_t* h, int cnt, F f) {
    MultiState& ms = *h->multi;
    for (int r = 0; r < cnt; ++r) ms.rep_worker[r]->post([&f, &ms, r]() -> int { return f(r, ms.rep[r]); });
    int rc = BPLTV_OK, bad = -1;
    for (int r = 0; r < cnt; ++r) {
        const int q = ms.rep_worker[r]->wait();
        if (q != BPLTV_OK && rc == BPLTV_OK) { rc = q; bad = r; }
    }
    if (rc != BPLTV_OK)
        set_err(h, rc, "replica %d (all %d images, device %d): %s", bad, h->O, ms.req_dev[bad], ms.rep[bad] ? ms.rep[bad]->err.c_str() : "creation failed");
    return rc;
}

// Make sure `want` replicas exist and hold the dataset.  A replica is an ordinary single-device handle over all O
// images; the dataset comes from the shards' resident copies through the host (once per bpltv_set_data -- the library
// keeps no host pointer of the caller's).
int multi_replicas_ready(bpltv_t* h, int want) {
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    const int have = (int)ms.rep.size();
    if (want > (int)ms.req_dev.size()) return set_err(h, BPLTV_E_ARG, "replicas: %d wanted, %zu devices requested", want, ms.req_dev.size());
    if (want > have) {
        for (int r = have; r < want; ++r) {
            ms.rep.push_back(nullptr);
            if (r < n) ms.rep_worker.push_back(ms.worker[r].get());
            else {
                ms.rep_owned.emplace_back(new ShardWorker(ms.req_dev[r]));
                ms.rep_worker.push_back(ms.rep_owned.back().get());
            }
        }
        const int M = h->M, N = h->N, O = h->O;
        int rc = rep_run(h, want, [&ms, M, N, O, n, have](int r, bpltv_t*) -> int {
            if (r < have) return BPLTV_OK;
            if (r == 0 && n == 1) { ms.rep[0] = ms.shard[0]; return BPLTV_OK; }   // one shard holds every image already
            const int rc2 = bpltv_create(&ms.rep[r], M, N, O, ms.req_dev[r], ms.dtype);
            if (rc2 == BPLTV_OK) ms.rep[r]->opt = ms.shard[0]->opt;
            return rc2;
        });
        if (rc) {   // leave no half-made replica behind: a later call starts from `have` again
            for (int r = want - 1; r >= have; --r) {
                bpltv_t* c = ms.rep[r];
                if (c && !(r == 0 && n == 1)) {
                    ms.rep_worker[r]->post([c]() -> int { (void)bpltv_destroy(c); return 0; });
                    (void)ms.rep_worker[r]->wait();
                }
                ms.rep.pop_back();
                ms.rep_worker.pop_back();
                if (r >= n) ms.rep_owned.pop_back();
            }
            return rc;
        }
        ms.rep_data = false;
        std::set<int> distinct(ms.dev.begin(), ms.dev.end());
        for (int r = 0; r < want; ++r) distinct.insert(ms.req_dev[r]);
        h->st.ngpus = (int)distinct.size();
    }
    if (!ms.rep_data) {
        if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
        std::vector<double> ub(h->tot), f(h->tot);
        const size_t npx = h->npx;
        int rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
            HIPCHK(c, hipMemcpy(ub.data() + ms.lo[k] * npx, c->d_ubar, c->tot * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(f.data() + ms.lo[k] * npx, c->d_f, c->tot * sizeof(double), hipMemcpyDeviceToHost));
            return BPLTV_OK;
        });
        if (rc) return rc;
        rc = rep_run(h, (int)ms.rep.size(), [&](int r, bpltv_t* c) { return (r == 0 && ms.rep_borrowed0()) ? BPLTV_OK : bpltv_set_data(c, ub.data(), f.data()); });
        if (rc) return rc;
        ms.rep_data = true;
    }
    return BPLTV_OK;
}

int multi_set_data(bpltv_t* h, const double* ubar, const double* f) {
    if (!ubar || !f) return set_err(h, BPLTV_E_ARG, "set_data: null pointer");
    MultiState& ms = *h->multi;
    const size_t npx = h->npx;
    int rc = multi_run(h, [&](int k, bpltv_t* c) { return bpltv_set_data(c, ubar + ms.lo[k] * npx, f + ms.lo[k] * npx); });
    if (rc) return rc;
    h->has_data = true;
    ms.rep_data = false;
    if (!ms.rep.empty()) {   // replicas exist already: they take the whole dataset from the caller's arrays
        rc = rep_run(h, (int)ms.rep.size(), [&](int r, bpltv_t* c) { return (r == 0 && ms.rep_borrowed0()) ? BPLTV_OK : bpltv_set_data(c, ubar, f); });
        if (rc) return rc;
        ms.rep_data = true;
    }
    return BPLTV_OK;
}

// each (bpltv_denoise_each, bpltv_sumregs_denoise_each): alpha holds O blocks of slices*am*an doubles; shard k takes the
// blocks [lo_k, hi_k).  Their entries are checked here first, so that a block one shard would reject does not leave the others' solves behind.
int multi_denoise(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out, int slices = 1,
                  bool each = false) {
    WallTimer wt;
    MultiState& ms = *h->multi;
    const size_t npx = h->npx, P = (size_t)slices * am * an;
    if (each) {
        if (!alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "alpha: null pointer or empty shape");
        const bpltv_params p = resolve(pp);
        double amin = 0.0;
        if (int crc = check_alpha_host(h, "alpha", alpha, (size_t)h->O * P, &amin)) return crc;
        if (p.rho != 0.0 && !(amin > 0.0))
            return set_err(h, BPLTV_E_ARG, "rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", amin);
    }
    int rc = multi_run(h, [&](int k, bpltv_t* c) {
        double* uo = u_out ? u_out + ms.lo[k] * npx : nullptr;
        if (each)
            return slices == 3 ? bpltv_sumregs_denoise_each(c, alpha + ms.lo[k] * P, am, an, pp, uo)
                               : bpltv_denoise_each(c, alpha + ms.lo[k] * P, am, an, pp, uo);
        return slices == 3 ? bpltv_sumregs_denoise(c, alpha, am, an, pp, uo) : bpltv_denoise(c, alpha, am, an, pp, uo);
    });
    if (rc) return rc;
    h->has_result = true;
    h->st.collective = 0; h->st.collective_ms = 0.0;
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

// tv_op_learning_function over the shards: every device evaluates its images, then ONE collective on the
// [cost, grad...] vector.  out: host, 1 + am*an doubles.
int multi_evaluate(bpltv_t* h, const double* alpha, int am, int an, double delta, const bpltv_params* pp,
                   double* u_out, double* out, int slices = 1) {
    WallTimer wt;
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    const size_t npx = h->npx, P = (size_t)am * an * slices, np = 1 + P;
    const bpltv_params p = resolve(pp);
    int rc = multi_run(h, [&](int k, bpltv_t* c) {
        double* uo = u_out ? u_out + ms.lo[k] * npx : nullptr;
        return evaluate_common(c, slices == 3, alpha, am, an, delta, pp, uo, nullptr, nullptr);
    });
    if (rc) return rc;
    const bool amap = (am == h->M && an == h->N) && !(h->M == 1 && h->N == 1);
    const bool ordered = p.deterministic != 0 && !amap;
    const bool rccl = !ms.comm.empty();
    WallTimer ct;
    if (ordered) {
        // per-image rows [cost_k, grad_k...] of every shard, added in global image order (plain left-to-right
        // sums == what sum_final_kernel does on one device): totals bitwise independent of the sharding
        std::vector<double> rows((size_t)n * ms.maxloc * np, 0.0);
        if (rccl) {
            const size_t need = (size_t)ms.maxloc * np;
            rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
                if (ms.rows_cap[k] < need) {
                    if (ms.d_rows[k]) (void)hipFree(ms.d_rows[k]);
                    if (ms.d_all[k]) (void)hipFree(ms.d_all[k]);
                    ms.d_rows[k] = ms.d_all[k] = nullptr;
                    ms.rows_cap[k] = 0;
                    const int arc = alloc_all(c, {{(void**)&ms.d_rows[k], need * sizeof(double)},
                                                  {(void**)&ms.d_all[k], need * n * sizeof(double)}}, "all-gather buffers");
                    if (arc) return arc;
                    ms.rows_cap[k] = need;
                }
                hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, c->stream, c->d_perimg,
                                   c->d_red, c->O, (int)P, ms.maxloc, ms.d_rows[k]);
                HIPCHK(c, hipGetLastError());
                return BPLTV_OK;
            });
            if (rc) return rc;
            NCCLCHK(h, ncclGroupStart());
            for (int k = 0; k < n; ++k)
                NCCLCHK(h, ncclAllGather(ms.d_rows[k], ms.d_all[k], need, ncclDouble, ms.comm[k], ms.shard[k]->stream));
            NCCLCHK(h, ncclGroupEnd());
            rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
                if (k == 0)
                    HIPCHK(c, hipMemcpyAsync(rows.data(), ms.d_all[0], rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                return BPLTV_OK;
            });
            if (rc) return rc;
            h->st.collective = 2;
        } else {
            rc = multi_run(h, [&](int k, bpltv_t* c) { return bpltv_per_image(c, rows.data() + (size_t)k * ms.maxloc * np); });
            if (rc) return rc;
            h->st.collective = 3;
        }
        // cost: sum_final_kernel adds per-image values in image order; gradient entry q likewise
        for (size_t e = 0; e < np; ++e) out[e] = 0.0;
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < ms.hi[k] - ms.lo[k]; ++i) {
                const double* r = rows.data() + ((size_t)k * ms.maxloc + i) * np;
                for (size_t e = 0; e < np; ++e) out[e] += r[e];
            }
    } else if (rccl) {
        // ONE ncclAllReduce(sum, f64) over xGMI, in place on the shards' partial vectors (every rank of this
        // single-process communicator is driven from the caller's thread, grouped)
        NCCLCHK(h, ncclGroupStart());
        for (int k = 0; k < n; ++k)
            NCCLCHK(h, ncclAllReduce(ms.shard[k]->d_partial, ms.shard[k]->d_partial, np, ncclDouble, ncclSum, ms.comm[k],
                                     ms.shard[k]->stream));
        NCCLCHK(h, ncclGroupEnd());
        rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
            if (k == 0)
                HIPCHK(c, hipMemcpyAsync(out, c->d_partial, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return BPLTV_OK;
        });
        if (rc) return rc;
        h->st.collective = 1;
    } else {
        // repeated devices (rehearsal): RCCL cannot hold two ranks on one device; same sum on the host
        std::vector<double> part((size_t)n * np);
        rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
            HIPCHK(c, hipMemcpy(part.data() + (size_t)k * np, c->d_partial, np * sizeof(double), hipMemcpyDeviceToHost));
            return BPLTV_OK;
        });
        if (rc) return rc;
        for (size_t e = 0; e < np; ++e) {
            double acc = part[e];
            for (int k = 1; k < n; ++k) acc += part[(size_t)k * np + e];
            out[e] = acc;
        }
        h->st.collective = n > 1 ? 3 : 0;
    }
    h->st.collective_ms = ct.ms();
    h->has_result = true;
    h->has_per_image = !amap;
    h->last_am = am; h->last_an = an; h->last_slices = slices;
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

int multi_gradient(bpltv_t* h, const double* u, const double* ubar, const double* alpha, int am, int an, int reg,
                   const bpltv_params* pp, double* grad_out) {
    if (!u || !ubar || !grad_out || !alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "gradient: null pointer or empty shape");
    WallTimer wt;
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    const size_t npx = h->npx, P = (size_t)am * an;
    std::vector<double> g((size_t)n * P);
    int rc = multi_run(h, [&](int k, bpltv_t* c) {
        return bpltv_gradient(c, u + ms.lo[k] * npx, ubar + ms.lo[k] * npx, alpha, am, an, reg, pp, g.data() + (size_t)k * P);
    });
    if (rc) return rc;
    for (size_t e = 0; e < P; ++e) {   // gradient wrappers sum per-image terms (TVLearningFunctionVec.jl:76-82,168-173)
        double acc = g[e];
        for (int k = 1; k < n; ++k) acc += g[(size_t)k * P + e];
        grad_out[e] = acc;
    }
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

// bpltv_vjp over the shards: images split as for the gradient, input-gradient slices written in place, the parameter
// gradients of the shards added in shard order.  slices: 1 TV (bpltv_vjp), 3 sum of regularisers (bpltv_sumregs_vjp).
// each (bpltv_vjp_each, bpltv_sumregs_vjp_each): shard k takes the parameter blocks [lo_k, hi_k) and writes their gradients
// in place.
int multi_vjp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp,
              const double* gu, double* grad_f_out, double* grad_alpha_out, int slices = 1, bool each = false) {
    if (!u || !gu || !alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "vjp: null pointer or empty shape");
    if (!grad_f_out && !grad_alpha_out) return set_err(h, BPLTV_E_ARG, "vjp: both outputs are NULL");
    WallTimer wt;
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    const size_t npx = h->npx, P = (size_t)slices * am * an;
    std::vector<double> g((size_t)n * P);
    int rc = multi_run(h, [&](int k, bpltv_t* c) {
        const size_t o0 = ms.lo[k] * npx;
        double* gf = grad_f_out ? grad_f_out + o0 : nullptr;
        if (each) {
            double* gak = grad_alpha_out ? grad_alpha_out + ms.lo[k] * P : nullptr;
            return slices == 3 ? bpltv_sumregs_vjp_each(c, u + o0, alpha + ms.lo[k] * P, am, an, reg, pp, gu + o0, gf, gak)
                               : bpltv_vjp_each(c, u + o0, alpha + ms.lo[k] * P, am, an, reg, pp, gu + o0, gf, gak);
        }
        double* ga = grad_alpha_out ? g.data() + (size_t)k * P : nullptr;
        return slices == 3 ? bpltv_sumregs_vjp(c, u + o0, alpha, am, an, reg, pp, gu + o0, gf, ga)
                           : bpltv_vjp(c, u + o0, alpha, am, an, reg, pp, gu + o0, gf, ga);
    });
    if (rc) return rc;
    if (grad_alpha_out && !each)
        for (size_t e = 0; e < P; ++e) {
            double acc = g[e];
            for (int k = 1; k < n; ++k) acc += g[(size_t)k * P + e];
            grad_alpha_out[e] = acc;
        }
    h->has_per_image = false;
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

// slices: 1 TV (bpltv_sweep), 3 sum of regularisers (bpltv_sumregs_sweep; 3*am*an doubles per parameter block)
int multi_sweep(bpltv_t* h, const double* alphas, int K, int am, int an, const bpltv_params* pp, double* cost_out,
                double* u_out, int slices = 1) {
    if (!alphas || !cost_out || K < 1) return set_err(h, BPLTV_E_ARG, "sweep: null pointer or K < 1");
    if (am < 1 || an < 1 || am > h->M || an > h->N) return set_err(h, BPLTV_E_ARG, "sweep: bad parameter shape %dx%d", am, an);
    WallTimer wt;
    MultiState& ms = *h->multi;
    const int n = (int)ms.shard.size();
    const size_t npx = h->npx;
    h->st.sweep_shards = 0;
    {
        // Which axis to split: the images (what the shards already hold: device k solves K x O_k problems) or the K
        // parameter blocks over replicas (device r solves K_r x O problems).  Automatic = the smaller largest share;
        // ties keep the image split (no second copy of the dataset).  The reference's sweeps
        // (/root/reference/src/BPLDenoising.jl:92-111,136-158,381-415) run on num_samples = 1 by default (:313), where
        // only the parameter axis can use more than one device.
        const int nrep = (int)std::min<size_t>(ms.req_dev.size(), (size_t)K);
        const long share_img = (long)K * ms.maxloc, share_par = (long)((K + nrep - 1) / nrep) * h->O;
        const bool by_par = ms.sweep_split == 2 || (ms.sweep_split == 0 && share_par < share_img);
        if (by_par && nrep >= 1 && !(n == 1 && nrep == 1)) {
            int rc = multi_replicas_ready(h, nrep);
            if (rc) return rc;
            const size_t npar = (size_t)am * an * slices;
            rc = rep_run(h, nrep, [&](int r, bpltv_t* c) -> int {
                int lo, hi;
                shard_range(K, nrep, r, &lo, &hi);
                // parameter-major outputs: replica r's blocks [lo, hi) are contiguous in cost_out and u_out
                double* uo = u_out ? u_out + (size_t)lo * h->O * npx : nullptr;
                return slices == 3 ? bpltv_sumregs_sweep(c, alphas + (size_t)lo * npar, hi - lo, am, an, pp, cost_out + lo, uo)
                                   : bpltv_sweep(c, alphas + (size_t)lo * npar, hi - lo, am, an, pp, cost_out + lo, uo);
            });
            if (rc) return rc;
            bpltv_stats_t a = ms.rep[0]->st;
            for (int r = 1; r < nrep; ++r) {
                const bpltv_stats_t& b = ms.rep[r]->st;
                a.tiles += b.tiles;
                a.launches = std::max(a.launches, b.launches);
                a.pdhg_ms = std::max(a.pdhg_ms, b.pdhg_ms);
                a.algorithmic_bytes += b.algorithmic_bytes;
                a.iterations = std::max(a.iterations, b.iterations);
                a.sweep_groups = std::max(a.sweep_groups, b.sweep_groups);
            }
            a.O = h->O; a.ngpus = h->st.ngpus; a.shards = h->st.shards; a.nccl_ranks = h->st.nccl_ranks;
            a.collective = 0; a.collective_ms = 0.0;
            a.sweep_shards = nrep;
            a.total_ms = wt.ms();
            h->st = a;
            return BPLTV_OK;
        }
    }
    std::vector<double> cost((size_t)n * K);
    std::vector<std::vector<double>> ubuf(n);
    int rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
        const size_t Ok = (size_t)(ms.hi[k] - ms.lo[k]);
        if (u_out) ubuf[k].resize((size_t)K * Ok * npx);
        double* co = cost.data() + (size_t)k * K;
        double* uo = u_out ? ubuf[k].data() : nullptr;
        const int r = slices == 3 ? bpltv_sumregs_sweep(c, alphas, K, am, an, pp, co, uo) : bpltv_sweep(c, alphas, K, am, an, pp, co, uo);
        if (r == BPLTV_OK && u_out)   // parameter-major [K][O][N][M]: this shard's images of every parameter block
            for (int q = 0; q < K; ++q)
                std::memcpy(u_out + ((size_t)q * h->O + ms.lo[k]) * npx, ubuf[k].data() + (size_t)q * Ok * npx, Ok * npx * sizeof(double));
        return r;
    });
    if (rc) return rc;
    for (int q = 0; q < K; ++q) {
        double acc = cost[q];
        for (int k = 1; k < n; ++k) acc += cost[(size_t)k * K + q];
        cost_out[q] = acc;
    }
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

// An entry point that takes or returns a device pointer, on a multi-device handle: ambiguous over several shards, forwarded
// (call(shard 0)) when one shard holds everything.  The shard's error text becomes the handle's; what a successful call
// leaves on the multi handle (has_result, has_data, multi_stats) is the caller's.
template <class F>
int multi_forward0(bpltv_t* h, const char* what, F call) {
    MultiState& ms = *h->multi;
    if (ms.shard.size() != 1)
        return set_err(h, BPLTV_E_UNSUPPORTED, "%s takes a device pointer, which is ambiguous on a handle over %zu shards; use the host-array entry points",
                       what, ms.shard.size());
    const int r = call(ms.shard[0]);
    if (r) h->err = ms.shard[0]->err;
    return r;
}
// ... of an entry point that solves: afterwards the multi handle has a result, and the shard's statistics are its own
template <class F>
int multi_forward0_solve(bpltv_t* h, const char* what, F call) {
    const int r = multi_forward0(h, what, call);
    if (r == BPLTV_OK) { h->has_result = true; multi_stats(h); }
    return r;
}

// The tail of a sweep (or of one group of it): the loss of every problem of the kb parameter blocks x O images in d_u against
// ubar[img % O], summed per parameter block on the host in image order (the order is in the last bit of cost_out);
// u to the host when u_out is given.  d_cost: kb * O doubles of scratch.
int sweep_tail(bpltv_t* h, const double* d_u, int kb, double* d_cost, double* cost_out, double* u_out) {
    const int nblk = 16, O = h->O, np = kb * O;
    int rc = ensure(h, &h->d_red, &h->red_cap, (size_t)np * nblk);
    if (rc) return rc;
    hipLaunchKernelGGL(cost_partial_mod_kernel, dim3(nblk, (unsigned)np), dim3(256), 0, h->stream, d_u, h->d_ubar, (int)h->npx, O,
                       h->d_red);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, h->stream, h->d_red, nblk, np, 0.5, d_cost, (double*)nullptr);
    HIPCHK(h, hipGetLastError());
    std::vector<double> per(np);
    HIPCHK(h, hipMemcpyAsync(per.data(), d_cost, (size_t)np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (u_out) HIPCHK(h, hipMemcpyAsync(u_out, d_u, (size_t)np * h->npx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < kb; ++k) {
        double sacc = 0.0;
        for (int i = 0; i < O; ++i) sacc += per[(size_t)k * O + i];
        cost_out[k] = sacc;
    }
    return BPLTV_OK;
}

// bpltv_vjp (slices = 1) and bpltv_sumregs_vjp (3): host arrays staged in d_u2 / d_ubar2 / d_gf2, the parameter gradient
// read back from d_vjp.
int vjp_host(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp,
             const double* gu, double* grad_f_out, double* grad_alpha_out, int slices, bool each = false) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_vjp(h, u, alpha, am, an, reg, pp, gu, grad_f_out, grad_alpha_out, slices, each);
    if (!u || !gu || !alpha) return set_err(h, BPLTV_E_ARG, "vjp: null pointer");
    if (!grad_f_out && !grad_alpha_out) return set_err(h, BPLTV_E_ARG, "vjp: both outputs are NULL");
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "vjp: parameter shape %dx%d (image %dx%d)", am, an, h->M, h->N);
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, h->tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, h->tot * sizeof(double)));
    }
    if (grad_f_out && !h->d_gf2) HIPCHK(h, hipMalloc((void**)&h->d_gf2, h->tot * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(h->d_u2, u, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar2, gu, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const size_t P = (size_t)slices * am * an * (each ? h->O : 1);
    int rc = ensure(h, &h->d_vjp, &h->vjp_cap, 4 + 2 * P);
    if (rc) return rc;
    double* d_ga = grad_alpha_out ? h->d_vjp + 4 + P : nullptr;
    rc = vjp_common(h, h->d_u2, alpha, false, am, an, reg, pp, h->d_ubar2, grad_f_out ? h->d_gf2 : nullptr, d_ga, slices, each);
    if (rc) return rc;
    if (grad_f_out)
        HIPCHK(h, hipMemcpyAsync(grad_f_out, h->d_gf2, h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_alpha_out)
        HIPCHK(h, hipMemcpyAsync(grad_alpha_out, d_ga, sizeof(double) * P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// bpltv_vjp_device (slices = 1) and bpltv_sumregs_vjp_device (3)
int vjp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg, const bpltv_params* pp,
               const double* d_gu, double* d_grad_f, double* d_grad_alpha, int slices, bool each = false) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) {
        const int r = multi_forward0(h, each ? (slices == 3 ? "bpltv_sumregs_vjp_each_device" : "bpltv_vjp_each_device") : (slices == 3 ? "bpltv_sumregs_vjp_device" : "bpltv_vjp_device"), [&](bpltv_t* c) {
            return vjp_device(c, d_u, d_alpha, am, an, reg, pp, d_gu, d_grad_f, d_grad_alpha, slices, each);
        });
        if (r == BPLTV_OK) { h->has_per_image = false; multi_stats(h); }   // no solve ran: has_result stays
        return r;
    }
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = vjp_common(h, d_u, d_alpha, true, am, an, reg, pp, d_gu, d_grad_f, d_grad_alpha, slices, each);
    if (rc) return rc;
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// bpltv_jvp / bpltv_jvp_each over the shards: images split as for the VJP.  The arrays are direction-major over the
// WHOLE batch, so every shard gets its images of every direction packed (and, each, its parameter blocks), and its du
// slices are scattered back in place: no reduction.  slices: 1 TV, 3 sum of regularisers (blocks of 3*am*an doubles).
int multi_jvp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp, int ndir,
              const double* df, const double* dalpha, double* du_out, bool each, int slices) {
    if (!u || !alpha || !du_out || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "jvp: null pointer or empty shape");
    if (ndir < 1) return set_err(h, BPLTV_E_ARG, "jvp: ndir = %d (at least one direction)", ndir);
    if (!df && !dalpha) return set_err(h, BPLTV_E_ARG, "jvp: both tangents are NULL");
    WallTimer wt;
    MultiState& ms = *h->multi;
    const size_t npx = h->npx, tot = h->tot, P = (size_t)slices * am * an;
    const bool sr = slices == 3;
    int rc = multi_run(h, [&](int k, bpltv_t* c) -> int {
        const size_t o0 = ms.lo[k] * npx, nk = (size_t)(ms.hi[k] - ms.lo[k]), tk = nk * npx;
        std::vector<double> dfk(df ? ndir * tk : 0), dak(dalpha && each ? ndir * nk * P : 0), duk(ndir * tk);
        for (int d = 0; d < ndir; ++d) {
            if (df) std::memcpy(dfk.data() + d * tk, df + d * tot + o0, tk * sizeof(double));
            if (dalpha && each) std::memcpy(dak.data() + d * nk * P, dalpha + ((size_t)d * h->O + ms.lo[k]) * P, nk * P * sizeof(double));
        }
        const double *ak = each ? alpha + ms.lo[k] * P : alpha, *dfp = df ? dfk.data() : nullptr;
        const double* dap = dalpha ? (each ? dak.data() : dalpha) : nullptr;
        const int r = each ? (sr ? bpltv_sumregs_jvp_each(c, u + o0, ak, am, an, reg, pp, ndir, dfp, dap, duk.data())
                                 : bpltv_jvp_each(c, u + o0, ak, am, an, reg, pp, ndir, dfp, dap, duk.data()))
                           : (sr ? bpltv_sumregs_jvp(c, u + o0, ak, am, an, reg, pp, ndir, dfp, dap, duk.data())
                                 : bpltv_jvp(c, u + o0, ak, am, an, reg, pp, ndir, dfp, dap, duk.data()));
        if (r == BPLTV_OK)
            for (int d = 0; d < ndir; ++d) std::memcpy(du_out + d * tot + o0, duk.data() + d * tk, tk * sizeof(double));
        return r;
    });
    if (rc) return rc;
    h->st.total_ms = wt.ms();
    return multi_stats(h);
}

// bpltv_jvp and bpltv_jvp_each: host arrays staged in d_u2 and d_jvp = [du | df | dalpha]
int jvp_host(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp, int ndir,
             const double* df, const double* dalpha, double* du_out, bool each, int slices = 1) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_jvp(h, u, alpha, am, an, reg, pp, ndir, df, dalpha, du_out, each, slices);
    if (!u || !alpha || !du_out) return set_err(h, BPLTV_E_ARG, "jvp: null pointer");
    if (ndir < 1) return set_err(h, BPLTV_E_ARG, "jvp: ndir = %d (at least one direction)", ndir);
    if (!df && !dalpha) return set_err(h, BPLTV_E_ARG, "jvp: both tangents are NULL");
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "jvp: parameter shape %dx%d (image %dx%d)", am, an, h->M, h->N);
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, h->tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, h->tot * sizeof(double)));
    }
    const size_t nt = (size_t)ndir * h->tot, na = (size_t)ndir * slices * am * an * (each ? h->O : 1);
    int rc = ensure(h, &h->d_jvp, &h->jvp_cap, 2 * nt + na);
    if (rc) return rc;
    double *d_du = h->d_jvp, *d_df = df ? h->d_jvp + nt : nullptr, *d_da = dalpha ? h->d_jvp + 2 * nt : nullptr;
    HIPCHK(h, hipMemcpyAsync(h->d_u2, u, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (df) HIPCHK(h, hipMemcpyAsync(d_df, df, nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (dalpha) HIPCHK(h, hipMemcpyAsync(d_da, dalpha, na * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = jvp_common(h, h->d_u2, alpha, false, am, an, reg, pp, ndir, d_df, d_da, d_du, each, slices);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(du_out, d_du, nt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// bpltv_jvp_device and bpltv_jvp_each_device
int jvp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg, const bpltv_params* pp, int ndir,
               const double* d_df, const double* d_dalpha, double* d_du, bool each, int slices = 1) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) {
        const char* name = slices == 3 ? (each ? "bpltv_sumregs_jvp_each_device" : "bpltv_sumregs_jvp_device")
                                       : (each ? "bpltv_jvp_each_device" : "bpltv_jvp_device");
        const int r = multi_forward0(h, name, [&](bpltv_t* c) {
            return jvp_device(c, d_u, d_alpha, am, an, reg, pp, ndir, d_df, d_dalpha, d_du, each, slices);
        });
        if (r == BPLTV_OK) multi_stats(h);   // no solve ran: has_result stays
        return r;
    }
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = jvp_common(h, d_u, d_alpha, true, am, an, reg, pp, ndir, d_df, d_dalpha, d_du, each, slices);
    if (rc) return rc;
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// bpltv_gauss_newton: gradient and Gauss-Newton Hessian of 0.5||u(alpha) - ubar||^2 from the P = slices*am*an <= GN_MAXP
// columns du/dalpha_j, solved as the unit directions of one jvp_common call (one factorisation per image group).
// slices: 1 TV, 3 sum of regularisers (bpltv_sumregs_gauss_newton; columns in the order of the parameter layout).
constexpr int GN_MAXP = 16;
int gauss_newton(bpltv_t* h, const double* u, const double* ubar, const double* alpha, int am, int an, int reg,
                 const bpltv_params* pp, double* grad_out, double* hess_out, int slices = 1) {
    if (!h) return BPLTV_E_ARG;
    if (!u || !ubar || !alpha || !grad_out || !hess_out) return set_err(h, BPLTV_E_ARG, "gauss_newton: null pointer");
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "gauss_newton: parameter shape %dx%d (image %dx%d)", am, an, h->M, h->N);
    const bool amap = am == h->M && an == h->N && !(h->M == 1 && h->N == 1);
    if (amap || (long)slices * am * an > GN_MAXP)
        return set_err(h, BPLTV_E_UNSUPPORTED, "gauss_newton: a scalar or a patch parameter of at most %d entries (got %s%dx%d%s); use bpltv_jvp for Jacobian columns",
                       GN_MAXP, slices == 3 ? "3 slices of " : "", am, an, amap ? ", a pixel map" : "");
    const int P = slices * am * an;
    const size_t nout = (size_t)P + (size_t)P * P;
    WallTimer wt;
    if (h->multi) {   // the shards' [grad, H] added on the host in shard order
        MultiState& ms = *h->multi;
        const int n = (int)ms.shard.size();
        std::vector<double> part((size_t)n * nout);
        const int rc = multi_run(h, [&](int k, bpltv_t* c) {
            double* o = part.data() + (size_t)k * nout;
            const double *uk = u + ms.lo[k] * h->npx, *bk = ubar + ms.lo[k] * h->npx;
            return slices == 3 ? bpltv_sumregs_gauss_newton(c, uk, bk, alpha, am, an, reg, pp, o, o + P)
                               : bpltv_gauss_newton(c, uk, bk, alpha, am, an, reg, pp, o, o + P);
        });
        if (rc) return rc;
        for (size_t e = 0; e < nout; ++e) {
            double acc = part[e];
            for (int k = 1; k < n; ++k) acc += part[(size_t)k * nout + e];
            (e < (size_t)P ? grad_out[e] : hess_out[e - P]) = acc;
        }
        h->st.total_ms = wt.ms();
        return multi_stats(h);
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, h->tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, h->tot * sizeof(double)));
    }
    // workspace [J: P planes | unit directions P x P | per-image partials P (P + 1) O | grad, H]
    const size_t nJ = (size_t)P * h->tot, npart = (size_t)P * (P + 1) * h->O;
    const size_t need = nJ + (size_t)P * P + npart + nout;
    if (h->jvp_cap < need) {
        if (h->d_jvp) (void)hipFree(h->d_jvp);
        h->d_jvp = nullptr; h->jvp_cap = 0;
        const int arc = alloc_all(h, {{(void**)&h->d_jvp, need * sizeof(double)}}, "gauss_newton: workspace of the Jacobian columns");
        if (arc) return arc;
        h->jvp_cap = need;
    }
    double *d_J = h->d_jvp, *d_e = d_J + nJ, *d_part = d_e + (size_t)P * P, *d_out = d_part + npart;
    std::vector<double> eye((size_t)P * P, 0.0);
    for (int j = 0; j < P; ++j) eye[(size_t)j * P + j] = 1.0;
    HIPCHK(h, hipMemcpyAsync(h->d_u2, u, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar2, ubar, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_e, eye.data(), eye.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (eye is a local)
    int rc = jvp_common(h, h->d_u2, alpha, false, am, an, reg, pp, P, nullptr, d_e, d_J, false, slices);
    if (rc) return rc;
    hipLaunchKernelGGL(gn_gram_kernel, dim3(P + 1, P, h->O), dim3(256), 0, h->stream, d_J, h->d_u2, h->d_ubar2, (int)h->npx, h->O, P,
                       d_part);
    hipLaunchKernelGGL(gn_final_kernel, dim3((P * (P + 1) + 63) / 64), dim3(64), 0, h->stream, d_part, h->O, P, d_out);
    HIPCHK(h, hipGetLastError());
    std::vector<double> out(nout);
    HIPCHK(h, hipMemcpyAsync(out.data(), d_out, nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(grad_out, out.data(), P * sizeof(double));
    std::memcpy(hess_out, out.data() + P, (size_t)P * P * sizeof(double));
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// ============================================================================================
// Per-pixel data-fidelity weight (weighted_kernels.hpp)
// ============================================================================================
// n entries of a weight array, finite and >= 0, on the host or (on_device) in HBM by alpha_check_kernel; *wmin receives the
// smallest.  Reads only: nothing of the handle changes.
int check_weight(bpltv_t* h, const char* who, const double* w, bool on_device, size_t n, double* wmin) {
    if (!on_device) {
        double mn = w[0];
        for (size_t e = 0; e < n; ++e) {
            if (!std::isfinite(w[e]) || w[e] < 0.0)
                return set_err(h, BPLTV_E_ARG, "%s: w[%zu] = %g: the fidelity weight must be finite and >= 0", who, e, w[e]);
            if (w[e] < mn) mn = w[e];
        }
        *wmin = mn;
        return BPLTV_OK;
    }
    int failed = -1;
    unsigned long long* chk = reinterpret_cast<unsigned long long*>(h->d_scalar + 2);
    if (int rc = check_device_arrays(h, chk, {w, n}, {}, wmin, &failed)) return rc;
    if (failed == 0) return set_err(h, BPLTV_E_ARG, "%s: w (device array): the fidelity weight must be finite and >= 0", who);
    return BPLTV_OK;
}

// The TV-KL model's dataset: finite and >= 0, by alpha_check_kernel on the resident f.  The answer is
// kept with the dataset (bpltv_set_data forgets it), so a dataset is reduced at most once.  Reads only, but for that memo.
int check_dataset_nonneg(bpltv_t* h, const char* who) {
    if (h->f_nonneg < 0) {
        int failed = -1;
        double fmin = 0.0;
        unsigned long long* chk = reinterpret_cast<unsigned long long*>(h->d_scalar + 2);
        if (int rc = check_device_arrays(h, chk, {h->d_f, h->tot}, {}, &fmin, &failed)) return rc;
        h->f_nonneg = failed == 0 ? 0 : 1;
    }
    if (!h->f_nonneg)
        return set_err(h, BPLTV_E_ARG, "%s: the dataset f has a negative or non-finite entry: the Kullback-Leibler data term needs f finite and >= 0", who);
    return BPLTV_OK;
}

// Tiling of a weighted solve: 32 x 32 regions, T iterations per launch (params.tile_iters, default 8; a halo must leave a
// core, and the kernel keeps at most PDHG_MAX_T step rows).  Results do not depend on T.
struct WeightedPlan { int T, nTi, nTj; };
int weighted_plan(bpltv_t* h, const bpltv_params& p, WeightedPlan* pl) {
    auto maxT = [](int L) { return (L <= TV_R) ? PDHG_MAX_T : (TV_R - 1) / 2; };
    int T = p.tile_iters > 0 ? p.tile_iters : 8;
    T = std::min(T, std::min(PDHG_MAX_T, std::min(maxT(h->M), maxT(h->N))));
    pl->T = T;
    pl->nTi = tile_count(h->M, TV_R, T);
    pl->nTj = tile_count(h->N, TV_R, T);
    if (pl->nTi < 1 || pl->nTj < 1) return set_err(h, BPLTV_E_ARG, "cannot tile %dx%d with T=%d", h->M, h->N, T);
    if (pl->nTj > 65535 || h->O > 65535 || (long long)pl->nTi * pl->nTj * h->O > 0x7FFFFFFFll)
        return set_err(h, BPLTV_E_UNSUPPORTED, "weighted solve: at most 65535 tile rows, 65535 images and 2^31 tiles per launch (grid dimensions)");
    return BPLTV_OK;
}

// What a weighted call rejects on its parameters alone
int weighted_check_params(bpltv_t* h, const bpltv_params& p, const char* who) {
    if (int prc = check_params(h, p)) return prc;
    if (p.rho != 0.0) return set_err(h, BPLTV_E_UNSUPPORTED, "%s: params.rho must be 0 (no Huber smoothing in the weighted model)", who);
    if (p.init != 0 || p.order != 0) return set_err(h, BPLTV_E_UNSUPPORTED, "%s: params.init / params.order must be 0", who);
    return BPLTV_OK;
}

// One launch of tv_tile_kernel.  The caller has set what its entry point owns -- the planes, alpha (and w), the tape, the
// tangents; here: what every launch has, and the instance (a tape means TAPE)
void tv_tile_launch(bpltv_t* h, const WeightedPlan& pl, const double* tab, const LaunchStep& s, bool weighted, bool tangent, TvTileArgs& a,
                    bool l1 = false, bool kl = false) {
    a.f = h->d_f; a.tab = tab;
    a.it0 = s.it; a.nit = s.nit;
    a.M = h->M; a.N = h->N; a.halo = pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(TvTileArgs) = tangent    ? (weighted ? &tv_tile_kernel<true, false, true> : &tv_tile_kernel<false, false, true>)
                               : a.tape   ? (weighted ? &tv_tile_kernel<true, true, false> : &tv_tile_kernel<false, true, false>)
                                          : (weighted ? &tv_tile_kernel<true, false, false> : &tv_tile_kernel<false, false, false>);
    if (l1) kern = tangent ? &tv_tile_kernel<true, false, true, true> : (a.tape ? &tv_tile_kernel<true, true, false, true> : &tv_tile_kernel<true, false, false, true>);   // (weighted)
    if (kl) kern = tangent ? &tv_tile_kernel<true, false, true, false, true>
                           : (a.tape ? &tv_tile_kernel<true, true, false, false, true> : &tv_tile_kernel<true, false, false, false, true>);
    hipLaunchKernelGGL(kern, dim3(pl.nTi, pl.nTj, s.hi - s.lo), dim3(TV_R * TV_R), tangent ? tv_tangent_lds_bytes() : tv_lds_bytes(), s.st, a);
}

// maxiter iterations of the weighted recurrence on the dataset images, in the TV state sets, with the handle's d_w / w_wo /
// w_min and d_alpha.  *result_buf: the state set that holds the result.
int run_weighted_pdhg(bpltv_t* h, const bpltv_params& p, const WeightedPlan& pl, int* result_buf) {
    h->has_per_image = false;
    double* d_tab = nullptr;
    int rc = get_table(h, p, &d_tab, 8.0, 0, h->w_min);
    if (rc) return rc;
    const int M = h->M, N = h->N, O = h->O, T = pl.T;
    const bool amap = (h->last_am == M && h->last_an == N) && !(M == 1 && N == 1);
    h->st.tile_iters = T; h->st.tiles = pl.nTi * pl.nTj * O; h->st.region_i = TV_R; h->st.region_j = TV_R; h->st.pdhg_variant = 0;
    ChainSolve j;
    j.model = MODEL_W; j.nplanes = 3; j.state0 = h->d_state[0];
    j.nimg = O; j.niter = p.maxiter; j.T = T;
    j.chains = plan_chains(p.reserved[1], h->st.tiles, h->ncu, O, 2);   // at most two (image groups on two streams)
    j.bytes_per_px_iter = amap ? 72.0 : 64.0;   // read x, y1, y2, f, w (+ alpha), write x, y1, y2
    j.key = GraphKey{p.maxiter, T, 0, h->last_am, h->last_an, j.chains, 0.0, 0.0, 0.0, 0, 0, 0, nullptr, (const void*)d_tab, 0,
                     (const void*)h->d_alpha, 0, h->w_wo};
    j.enqueue = launch_loop(T, [&](const LaunchStep& s) {
        TvTileArgs a{};
        for (int c = 0; c < 3; ++c) { a.in[c] = h->d_state[s.cur][c]; a.out[c] = h->d_state[s.nxt][c]; }
        a.w = h->d_w; a.wstride = h->w_wo > 1 ? h->npx : 0;
        a.alpha = h->d_alpha; a.am = h->last_am; a.an = h->last_an;
        tv_tile_launch(h, pl, d_tab, s, true, false, a);
    });
    return run_chains(h, p, j, result_buf);   // (no gap callback: the weighted solve does not take params.check_every)
}

// bpltv_weighted_denoise(_device) on a single-device handle: w and the parameter from the host or (dev) from HBM.  The
// order is the contract: arguments, params, w, then upload_alpha (shape, values, what the solve would reject) -- and only
// then the handle's copy of w.
int weighted_denoise_common(bpltv_t* h, const double* w, int wo, const double* alpha, bool dev, int am, int an,
                            const bpltv_params* pp, double* u_out) {
    const char* who = dev ? "bpltv_weighted_denoise_device" : "bpltv_weighted_denoise";
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    if (!w) return set_err(h, BPLTV_E_ARG, "%s: w is a null pointer", who);
    if (wo != 1 && wo != h->O) return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, wo, h->O);
    const bpltv_params p = resolve(pp);
    if (int prc = weighted_check_params(h, p, who)) return prc;
    WeightedPlan pl;
    if (int prc = weighted_plan(h, p, &pl)) return prc;
    const size_t nw = (size_t)wo * h->npx;
    double wmin = 0.0;
    int rc = check_weight(h, who, w, dev, nw, &wmin);
    if (rc) return rc;
    if (!h->d_w) {
        rc = alloc_all(h, {{(void**)&h->d_w, h->tot * sizeof(double)}}, "fidelity weight");
        if (rc) return rc;
    }
    bpltv_params q = p;   // the TV planner's knobs mean nothing here: upload_alpha's precheck sees the defaults
    q.tile_iters = 0; q.reserved[0] = 0; q.reserved[1] = 0; q.reserved[2] = 0;
    rc = upload_alpha(h, alpha, dev, am, an, PRE_TV, 1, &q);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_w, w, nw * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    h->w_wo = wo;
    h->w_min = wmin;
    int buf = 0;
    rc = run_weighted_pdhg(h, p, pl, &buf);
    if (rc) return rc;
    h->result_buf = buf;
    h->has_result = true;
    h->last_is_sr = false;
    h->last_weighted = true;
    h->last_channels = 0;
    h->last_l1 = false;
    h->last_kl = false;
    if (u_out) {
        HIPCHK(h, hipMemcpyAsync(u_out, h->d_state[buf][0], h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// bpltv_weighted_vjp(_device) on a single-device handle: d_u, d_f (nullable unless d_grad_w), d_gu and the outputs live in
// HBM; w and alpha on the host or (dev) in HBM.  Checks and staging by stage_param: nothing of the handle changes on a
// rejection, and the last solve's d_alpha and d_w stay as they were.
int weighted_vjp_common(bpltv_t* h, const double* d_u, const double* d_f, const double* w, int wo, const double* alpha, bool dev,
                        int am, int an, const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha,
                        double* d_grad_w) {
    const char* who = "weighted_vjp";
    if (!d_u || !w || !alpha || !d_gu) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (!d_grad_f && !d_grad_alpha && !d_grad_w) return set_err(h, BPLTV_E_ARG, "%s: all three outputs are NULL", who);
    if (d_grad_w && !d_f) return set_err(h, BPLTV_E_ARG, "%s: grad_w = -(u - f) o p needs f", who);
    if (wo != 1 && wo != h->O) return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, wo, h->O);
    bpltv_params p;
    GradCtx g;
    if (int rc = stage_param(h, who, alpha, dev, am, an, 1, false, 0, pp, w, wo, {{d_gu, h->tot, "cotangent gu"}}, &p, &g)) return rc;
    g.src = d_gu; g.cot = true;
    g.d_out = d_grad_alpha; g.d_grad_f = d_grad_f;
    g.f = d_f; g.d_grad_w = d_grad_w;
    h->has_per_image = false;
    return run_gradient(h, d_u, g, 0, p);
}

// a weighted or unrolled entry point on a multi-device handle: forwarded when one shard holds everything, unsupported otherwise
template <class F>
int weighted_multi(bpltv_t* h, const char* what, bool solve, F call, const char* model = "the weighted model") {
    MultiState& ms = *h->multi;
    if (ms.shard.size() != 1)
        return set_err(h, BPLTV_E_UNSUPPORTED, "%s: %s runs on single-device handles (this one has %zu shards)", what, model, ms.shard.size());
    const int r = call(ms.shard[0]);
    if (r) { h->err = ms.shard[0]->err; return r; }
    if (solve) h->has_result = true; else h->has_per_image = false;
    multi_stats(h);
    return r;
}

// ============================================================================================
// Reverse mode through the PDHG iterations (tv_tile_kernels.hpp, sumregs_unrolled_kernels.hpp;
// DESIGN.md sections 4.6, 4.8 and 4.9)
// ============================================================================================
EnqueueFn launch_loop(int T, LaunchFn launch) {
    return [T, launch](hipStream_t st, int it0, int it1, int cur, int lo, int hi, bool stagger) {
        int step = stagger ? T / 2 : T;
        for (int it = it0; it < it1; it += step, step = T) {
            const int nxt = (it == 0) ? (stagger ? 1 : 0) : 1 - cur;
            launch(LaunchStep{st, it, std::min(step, it1 - it), cur, nxt, (it == 0) ? 1 : 0, lo, hi});
            cur = nxt;
        }
        return cur;
    };
}

// What an unrolled call rejects on its parameters alone
int unrolled_check_params(bpltv_t* h, const bpltv_params& p, const char* who) {
    if (int prc = check_params(h, p)) return prc;
    if (p.rho != 0.0) return set_err(h, BPLTV_E_UNSUPPORTED, "%s: params.rho must be 0 (the taped recurrence has no Huber smoothing)", who);
    if (p.init != 0 || p.order != 0) return set_err(h, BPLTV_E_UNSUPPORTED, "%s: params.init / params.order must be 0", who);
    if (p.maxiter < 1) return set_err(h, BPLTV_E_ARG, "%s: maxiter = %d (at least one iteration)", who, p.maxiter);
    return BPLTV_OK;
}

// weighted_plan with the fusion depth capped at `cap` (the reverse kernel holds TV_REV_T iterations of tape in registers)
int unrolled_plan(bpltv_t* h, const bpltv_params& p, int cap, WeightedPlan* pl) {
    bpltv_params q = p;
    q.tile_iters = std::min(p.tile_iters > 0 ? p.tile_iters : 8, cap);
    return weighted_plan(h, q, pl);
}

// run_sr_pdhg's cut of the image into 32 x 32 regions (halo 2T, default T = 4), with the fusion depth capped at `cap` (the
// reverse kernel holds SRUN_REV_T iterations of tape in registers); the first use sets the kernels' LDS size
int sr_unrolled_plan(bpltv_t* h, const bpltv_params& p, int cap, WeightedPlan* pl) {
    if (p.tile_iters < 0) return set_err(h, BPLTV_E_ARG, "tile_iters must be >= 0");
    auto maxT = [](int L) { return (L <= SRUN_R) ? (1 << 20) : (SRUN_R - 1) / 4; };   // 2 * halo = 4T must leave a core
    pl->T = std::min(std::min(p.tile_iters > 0 ? p.tile_iters : 4, cap), std::min(maxT(h->M), maxT(h->N)));
    pl->nTi = tile_count(h->M, SRUN_R, 2 * pl->T);
    pl->nTj = tile_count(h->N, SRUN_R, 2 * pl->T);
    if (pl->T < 1 || pl->nTi < 1 || pl->nTj < 1) return set_err(h, BPLTV_E_ARG, "cannot tile %dx%d with T=%d", h->M, h->N, pl->T);
    if (h->O > 65535) return set_err(h, BPLTV_E_UNSUPPORTED, "the sum-of-regularisers solve takes at most 65535 problems per launch (problems are a grid dimension)");
    if (!h->srun_ready) {
        for (auto k : {&sr_unrolled_tile_kernel<SR_SHARED, true>, &sr_unrolled_tile_kernel<SR_EACH, true>, &sr_unrolled_tile_kernel<SR_SHARED, false>,
                       &sr_unrolled_tile_kernel<SR_EACH, false>})
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sr_lds_bytes(SRUN_R, SRUN_R)));
        for (auto k : {&sr_unrolled_reverse_tile_kernel<SR_SHARED>, &sr_unrolled_reverse_tile_kernel<SR_EACH>})
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sr_lds_bytes(SRUN_R, SRUN_R)));
        h->srun_ready = true;
    }
    return BPLTV_OK;
}

// What one launch of a taped solve reads besides the resident f: its two state sets, the parameter (and weight) and the tape --
// the handle's last ones for a solve, planes of its own, the staged parameter and the segment tape for the recompute of a
// checkpointed sweep.  tape == nullptr: the no-tape instantiation (the checkpoint pass) ...
struct TapedFwd {
    bpltv_t* h;
    WeightedPlan pl;
    const double* tab;
    double* tape;
    double* S[2][7];
    const double* alpha;
    int am, an;
    int astride;         // doubles between per-image parameter blocks (0: one block for every image)
    const double* w;     // weighted model; nullptr otherwise
    int wo;
    int channels = 1;    // channel-coupled model: planes of a colour image
    bool l1 = false;     // TV-L1 model: the weighted launch with the L1 primal step
    bool kl = false;     // TV-KL model: the weighted launch with the KL primal step
};
// the planes a launch reads and writes: a state set, or the step's checkpoint slot
static void taped_planes(const LaunchStep& s, int np, size_t tot, double* const (*S)[7], const double** in, double** out) {
    for (int c = 0; c < np; ++c) {
        in[c] = s.ckin ? s.ckin + (size_t)c * tot : S[s.cur][c];
        out[c] = s.ckout ? s.ckout + (size_t)c * tot : S[s.nxt][c];
    }
}
// ... and one launch of a reverse sweep: the staged parameter (and weight) g, the sweep's planes S | gf | ga | g0 (the cotangent,
// which the first launch reads in place of S[cur][0]) and gw (nullptr: not wanted), K = maxiter
struct TapedRev {
    bpltv_t* h;
    WeightedPlan pl;
    const double* tab;
    const double* tape;
    const GradCtx* g;
    double* S[2][7];
    double *gf, *ga, *g0, *gw;
    int K;
    int channels = 1;    // channel-coupled model: planes of a colour image
    bool l1 = false;     // TV-L1 model: the weighted launch with the L1 tail
    bool kl = false;     // TV-KL model: the weighted launch with the KL tail
};

// A model whose iterations can be taped and swept backwards: everything the two shared drivers (taped_denoise, taped_vjp)
// need to know about it.  The instances follow; a further model is one more of them and its kernels.
struct TapedModel {
    const char* denoise;          // stem of the solve's entry points ("_each", "_device" are appended), in messages
    const char* vjp;              // ... of the sweep's
    const char* tape_kind;        // "", "weighted ", ...: what a message calls its tape
    const char* multi_name;       // what weighted_multi's message calls these entry points
    Tape bpltv_handle::* tape;    // the handle's tape of this model
    int tape_planes;              // doubles per pixel and iteration on the tape
    int slices;                   // parameter slices: 1, or 3 (sum of regularisers: its defaults, PRE_SR, the d_sr state sets)
    bool weighted;                // takes a fidelity weight w: checked and staged, gamma = min w in the step table, grad_w
    bool l1;                      // TV-L1 model: weighted's plumbing with gamma = 0 whatever w is (no strong convexity), a sweep
                                  // that always reads the resident f, and no duality gap after its solves
    bool kl;                      // TV-KL model: the same, and a dataset that must be finite and >= 0
    bool flat() const { return l1 || kl; }   // no strong convexity: gamma = 0, omega = 1, constant steps
    int channels;                 // channel-coupled model: the planes of a colour image, which the launch chains keep together
                                  // and the handle's tape remembers (0: every plane is an image of its own)
    int nplanes;                  // planes of a state set
    double L2;                    // squared operator norm of the step table
    int (*plan)(bpltv_t*, const bpltv_params&, int cap, WeightedPlan*);
    int fwd_cap, rev_cap;         // deepest fusion of the taped solve / of the reverse sweep
    Model graphs;                 // graph cache, with the GraphKey variants of the solve and of the sweep (+ 1 with grad_w)
    int fwd_variant, rev_variant;
    int region;                   // statistics: region_i = region_j
    double bytes, bytes_map;      // bytes_per_px_iter of the solve with a scalar or patch parameter / with a map
    double plain_bytes, plain_bytes_map;   // ... of the model's plain solve: the checkpoint pass writes no tape
    double* bpltv_handle::* sweep;   // the reverse sweep's planes [2 sets x nplanes | gf | slices x ga | gu], allocated on first use
    const char* sweep_name;
    int adjoint_method;
    bool tv_stats;                // the sweep resets every adjoint statistic and its entry points set total_ms (TV), or it
                                  // changes adjoint_ms and adjoint_method only
    void (*launch_fwd)(const TapedFwd&, const LaunchStep&);
    void (*launch_rev)(const TapedRev&, const LaunchStep&);
};

void tv_launch_fwd(const TapedFwd& x, const LaunchStep& s) {   // x.w != nullptr: the weighted model
    bpltv_t* h = x.h;
    TvTileArgs a{};
    taped_planes(s, 3, h->tot, x.S, a.in, a.out);
    a.w = x.w; a.wstride = x.wo > 1 ? h->npx : 0;
    a.alpha = x.alpha; a.am = x.am; a.an = x.an; a.istride = x.astride;
    a.tape = x.tape; a.plane = h->tot; a.tk0 = s.tk0;
    tv_tile_launch(h, x.pl, x.tab, s, x.w != nullptr, false, a, x.l1, x.kl);
}
// `it` counts reverse steps: step r undoes iteration K - 1 - r.  g.w != nullptr: the weighted model (its kernel reads the
// resident f for gw only)
void tv_launch_rev(const TapedRev& x, const LaunchStep& s) {
    const GradCtx& g = *x.g;
    TvTileRevArgs a{};
    for (int c = 0; c < 3; ++c) { a.in[c] = x.S[s.cur][c]; a.out[c] = x.S[s.nxt][c]; }
    if (s.first) a.in[0] = x.g0;
    a.gf = x.gf; a.ga = x.ga; a.gw = x.gw; a.tape = x.tape; a.f = x.h->d_f; a.w = g.w; a.alpha = g.alpha; a.tab = x.tab;
    a.plane = x.h->tot; a.wstride = g.wo > 1 ? x.h->npx : 0;
    a.am = g.am; a.an = g.an; a.istride = g.astride;
    a.khi = x.K - 1 - s.it; a.nit = s.nit; a.tk0 = s.tk0;
    a.M = x.h->M; a.N = x.h->N; a.halo = x.pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(TvTileRevArgs) = x.l1 ? &tv_reverse_tile_kernel<true, true> : (g.w ? &tv_reverse_tile_kernel<true> : &tv_reverse_tile_kernel<false>);
    if (x.kl) kern = &tv_reverse_tile_kernel<true, false, true>;
    hipLaunchKernelGGL(kern, dim3(x.pl.nTi, x.pl.nTj, s.hi - s.lo), dim3(TV_R * TV_R), tv_lds_bytes(), s.st, a);
}

void sr_launch_fwd(const TapedFwd& x, const LaunchStep& s) {   // astride != 0: one parameter block per image
    bpltv_t* h = x.h;
    SrUnrolledArgs a;
    taped_planes(s, 7, h->tot, x.S, a.in, a.out);
    a.f = h->d_f; a.alpha = x.alpha; a.tab = x.tab; a.tape = x.tape; a.plane = h->tot;
    a.am = x.am; a.an = x.an; a.astride = x.astride;
    a.it0 = s.it; a.nit = s.nit; a.tk0 = s.tk0;
    a.M = h->M; a.N = h->N; a.halo = 2 * x.pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(SrUnrolledArgs) = x.astride != 0 ? (x.tape ? &sr_unrolled_tile_kernel<SR_EACH, true> : &sr_unrolled_tile_kernel<SR_EACH, false>)
                                                  : (x.tape ? &sr_unrolled_tile_kernel<SR_SHARED, true> : &sr_unrolled_tile_kernel<SR_SHARED, false>);
    hipLaunchKernelGGL(kern, dim3(x.pl.nTi, x.pl.nTj, s.hi - s.lo), dim3(SRUN_R * SRUN_R), sr_lds_bytes(SRUN_R, SRUN_R), s.st, a);
}
void sr_launch_rev(const TapedRev& x, const LaunchStep& s) {
    const GradCtx& g = *x.g;
    SrUnrolledRevArgs a;
    for (int c = 0; c < 7; ++c) { a.in[c] = x.S[s.cur][c]; a.out[c] = x.S[s.nxt][c]; }
    if (s.first) a.in[0] = x.g0;
    a.gf = x.gf; a.ga = x.ga; a.tape = x.tape; a.alpha = g.alpha; a.tab = x.tab; a.plane = x.h->tot;
    a.am = g.am; a.an = g.an; a.astride = g.astride;
    a.khi = x.K - 1 - s.it; a.nit = s.nit; a.tk0 = s.tk0;
    a.M = x.h->M; a.N = x.h->N; a.halo = 2 * x.pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(SrUnrolledRevArgs) = g.each ? &sr_unrolled_reverse_tile_kernel<SR_EACH> : &sr_unrolled_reverse_tile_kernel<SR_SHARED>;
    hipLaunchKernelGGL(kern, dim3(x.pl.nTi, x.pl.nTj, s.hi - s.lo), dim3(SRUN_R * SRUN_R), sr_lds_bytes(SRUN_R, SRUN_R), s.st, a);
}

// bytes / bytes_map: read x, y1, y2, f (+ alpha), write x, y1, y2 and z1, z2
const TapedModel kTapedTV = [] {
    TapedModel m{};
    m.denoise = "bpltv_unrolled_denoise"; m.vjp = "unrolled_vjp"; m.tape_kind = ""; m.multi_name = "the unrolled solve";
    m.tape = &bpltv_handle::tape; m.tape_planes = 2;
    m.slices = 1; m.weighted = false; m.nplanes = 3; m.L2 = 8.0;
    m.plan = unrolled_plan; m.fwd_cap = PDHG_MAX_T; m.rev_cap = TV_REV_T;
    m.graphs = MODEL_UN; m.fwd_variant = 0; m.rev_variant = 1;
    m.region = TV_R; m.bytes = 72.0; m.bytes_map = 80.0; m.plain_bytes = 56.0; m.plain_bytes_map = 64.0;
    m.sweep = &bpltv_handle::d_unr; m.sweep_name = "reverse sweep";
    m.adjoint_method = 7; m.tv_stats = true;
    m.launch_fwd = tv_launch_fwd; m.launch_rev = tv_launch_rev;
    return m;
}();
// ... the same, and read w and write x onto the tape as well.  The sweep runs in the TV sweep's planes.
const TapedModel kTapedWeighted = [] {
    TapedModel m = kTapedTV;
    m.denoise = "bpltv_weighted_unrolled_denoise"; m.vjp = "weighted_unrolled_vjp"; m.tape_kind = "weighted ";
    m.multi_name = "the weighted unrolled solve";
    m.tape = &bpltv_handle::wtape; m.tape_planes = 3;
    m.weighted = true;
    m.fwd_variant = 6; m.rev_variant = 7;
    m.bytes = 88.0; m.bytes_map = 96.0; m.plain_bytes = 64.0; m.plain_bytes_map = 72.0;
    m.adjoint_method = 9; m.tv_stats = false;
    return m;
}();
// The TV-L1 model: the weighted model's plumbing, tape layout, sweep planes and traffic -- read x, y1,
// y2, f, w (+ alpha), write x, y1, y2 and z1, z2, x+ -- with a tape of its own and graph variants of its own under MODEL_UN:
// 20 = taped solve, 22 = plain solve, 23 / 24 = reverse sweep without / with grad_w.
const TapedModel kTapedL1 = [] {
    TapedModel m = kTapedWeighted;
    m.denoise = "bpltv_lone_unrolled_denoise"; m.vjp = "l1_unrolled_vjp"; m.tape_kind = "L1 ";
    m.multi_name = "the TV-L1 solve";
    m.tape = &bpltv_handle::l1tape;
    m.l1 = true;
    m.fwd_variant = 20; m.rev_variant = 23;
    m.adjoint_method = 15;
    return m;
}();
// The TV-KL model: as the TV-L1 model, with a tape of its own and graph variants of its own under
// MODEL_UN: 30 = taped solve, 32 = plain solve, 33 / 34 = reverse sweep without / with grad_w.
const TapedModel kTapedKL = [] {
    TapedModel m = kTapedWeighted;
    m.denoise = "bpltv_kl_unrolled_denoise"; m.vjp = "kl_unrolled_vjp"; m.tape_kind = "KL ";
    m.multi_name = "the TV-KL solve";
    m.tape = &bpltv_handle::kltape;
    m.kl = true;
    m.fwd_variant = 30; m.rev_variant = 33;
    m.adjoint_method = 16;
    return m;
}();
// ... read x, 6 y, f (+ 3 alpha), write x, 6 y and the 6 z
const TapedModel kTapedSr = [] {
    TapedModel m{};
    m.denoise = "bpltv_sumregs_unrolled_denoise"; m.vjp = "sumregs_unrolled_vjp"; m.tape_kind = "sum-of-regularisers ";
    m.multi_name = "the sum-of-regularisers unrolled solve";
    m.tape = &bpltv_handle::srtape; m.tape_planes = 6;
    m.slices = 3; m.weighted = false; m.nplanes = 7; m.L2 = 18.0;
    m.plan = sr_unrolled_plan; m.fwd_cap = (SRUN_R - 1) / 4; m.rev_cap = SRUN_REV_T;
    m.graphs = MODEL_SRUN; m.fwd_variant = 0; m.rev_variant = 1;
    m.region = SRUN_R; m.bytes = 168.0; m.bytes_map = 192.0; m.plain_bytes = 120.0; m.plain_bytes_map = 144.0;
    m.sweep = &bpltv_handle::d_srunr; m.sweep_name = "sum-of-regularisers reverse sweep";
    m.adjoint_method = 10; m.tv_stats = false;
    m.launch_fwd = sr_launch_fwd; m.launch_rev = sr_launch_rev;
    return m;
}();
const char* const kUnrolled = kTapedTV.multi_name;   // (the tangent sweep's entry points)

// The channel-coupled model (color_tile_kernels.hpp): the TV model's planes, tape layout, step table and sweep planes; the
// launches count colour images (s.lo, s.hi) and one workgroup holds the C planes of its colour image.  channels = 1 is the TV
// model: its kernels run.  x.w / g.w != nullptr: the weighted form, whose channels = 1 is the weighted
// TV model.
template <int C>
void color_launch_fwd_c(const TapedFwd& x, const LaunchStep& s, TvTileArgs& a) {
    void (*kern)(TvTileArgs) = x.w ? (x.tape ? &color_tile_kernel<C, true, true> : &color_tile_kernel<C, false, true>)
                                   : (x.tape ? &color_tile_kernel<C, true> : &color_tile_kernel<C, false>);
    hipLaunchKernelGGL(kern, dim3(x.pl.nTi, x.pl.nTj, s.hi - s.lo), dim3(TV_R * TV_R), color_lds_bytes(C), s.st, a);
}
void color_launch_fwd(const TapedFwd& x, const LaunchStep& s) {
    if (x.channels == 1) return tv_launch_fwd(x, s);
    bpltv_t* h = x.h;
    TvTileArgs a{};
    taped_planes(s, 3, h->tot, x.S, a.in, a.out);
    a.f = h->d_f; a.alpha = x.alpha; a.am = x.am; a.an = x.an; a.tab = x.tab;
    a.w = x.w; a.wstride = x.wo > 1 ? h->npx : 0;
    a.tape = x.tape; a.plane = h->tot; a.tk0 = s.tk0;
    a.it0 = s.it; a.nit = s.nit;
    a.M = h->M; a.N = h->N; a.halo = x.pl.T; a.first = s.first; a.img0 = s.lo;
    if (x.channels == 2) color_launch_fwd_c<2>(x, s, a);
    else if (x.channels == 3) color_launch_fwd_c<3>(x, s, a);
    else color_launch_fwd_c<4>(x, s, a);
}
void color_launch_rev(const TapedRev& x, const LaunchStep& s) {
    if (x.channels == 1) return tv_launch_rev(x, s);
    const GradCtx& g = *x.g;
    TvTileRevArgs a{};
    for (int c = 0; c < 3; ++c) { a.in[c] = x.S[s.cur][c]; a.out[c] = x.S[s.nxt][c]; }
    if (s.first) a.in[0] = x.g0;
    a.gf = x.gf; a.ga = x.ga; a.tape = x.tape; a.alpha = g.alpha; a.tab = x.tab;
    a.gw = x.gw; a.f = x.h->d_f; a.w = g.w;
    a.plane = x.h->tot; a.wstride = g.wo > 1 ? x.h->npx : 0;
    a.am = g.am; a.an = g.an;
    a.khi = x.K - 1 - s.it; a.nit = s.nit; a.tk0 = s.tk0;
    a.M = x.h->M; a.N = x.h->N; a.halo = x.pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(TvTileRevArgs) = x.channels == 2 ? &color_reverse_tile_kernel<2> : (x.channels == 3 ? &color_reverse_tile_kernel<3> : &color_reverse_tile_kernel<4>);
    if (g.w) kern = x.channels == 2 ? &color_reverse_tile_kernel<2, true> : (x.channels == 3 ? &color_reverse_tile_kernel<3, true> : &color_reverse_tile_kernel<4, true>);
    hipLaunchKernelGGL(kern, dim3(x.pl.nTi, x.pl.nTj, s.hi - s.lo), dim3(TV_R * TV_R), color_lds_bytes(x.channels), s.st, a);
}
// unrolled_plan; the first use raises the LDS the colour kernels may take (three and four sets of planes pass 64 KB)
int color_plan(bpltv_t* h, const bpltv_params& p, int cap, WeightedPlan* pl) {
    if (int prc = unrolled_plan(h, p, cap, pl)) return prc;
    if (!h->color_ready) {
        const void* k2[] = {(const void*)&color_tile_kernel<2, true>, (const void*)&color_tile_kernel<2, false>, (const void*)&color_reverse_tile_kernel<2>,
                            (const void*)&color_tile_kernel<2, true, true>, (const void*)&color_tile_kernel<2, false, true>,
                            (const void*)&color_reverse_tile_kernel<2, true>};
        const void* k3[] = {(const void*)&color_tile_kernel<3, true>, (const void*)&color_tile_kernel<3, false>, (const void*)&color_reverse_tile_kernel<3>,
                            (const void*)&color_tile_kernel<3, true, true>, (const void*)&color_tile_kernel<3, false, true>,
                            (const void*)&color_reverse_tile_kernel<3, true>};
        const void* k4[] = {(const void*)&color_tile_kernel<4, true>, (const void*)&color_tile_kernel<4, false>, (const void*)&color_reverse_tile_kernel<4>,
                            (const void*)&color_tile_kernel<4, true, true>, (const void*)&color_tile_kernel<4, false, true>,
                            (const void*)&color_reverse_tile_kernel<4, true>};
        for (const void* k : k2) HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_lds_bytes(2)));
        for (const void* k : k3) HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_lds_bytes(3)));
        for (const void* k : k4) HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_lds_bytes(4)));
        h->color_ready = true;
    }
    return BPLTV_OK;
}
// bytes: TV's per plane; the map's 8 bytes are read once for the C planes of a colour image
TapedModel taped_color(int C) {
    TapedModel m = kTapedTV;
    m.denoise = "bpltv_color_unrolled_denoise"; m.vjp = "color_unrolled_vjp"; m.tape_kind = "colour ";
    m.multi_name = "the channel-coupled solve";
    m.tape = &bpltv_handle::ctape;
    m.channels = C;
    m.plan = color_plan; m.rev_cap = color_rev_t(C);
    m.graphs = MODEL_COLOR; m.fwd_variant = 10 * C; m.rev_variant = 10 * C + 1;
    m.bytes_map = 72.0 + 8.0 / C; m.plain_bytes_map = 56.0 + 8.0 / C;
    m.adjoint_method = 12; m.tv_stats = false;
    m.launch_fwd = color_launch_fwd; m.launch_rev = color_launch_rev;
    return m;
}
const TapedModel kTapedColor[COLOR_MAX_C] = {taped_color(1), taped_color(2), taped_color(3), taped_color(4)};
// Its weighted form: the weighted model's tape layout, weight and gamma in the step table, and a shallower
// sweep.  bytes: the weighted model's per plane.  Graph variants of its own, 100 + 10 * C + 0 = taped solve, + 2 = plain solve,
// + 3 = reverse sweep, + 4 = with grad_w: no graph is shared with the colour model's 10 * C + 0 ... 6.
TapedModel taped_color_weighted(int C) {
    TapedModel m = taped_color(C);
    m.denoise = "bpltv_color_weighted_unrolled_denoise"; m.vjp = "color_weighted_unrolled_vjp"; m.tape_kind = "colour-weighted ";
    m.multi_name = "the weighted channel-coupled solve";
    m.tape = &bpltv_handle::cwtape; m.tape_planes = 3;
    m.weighted = true;
    m.rev_cap = color_weighted_rev_t(C);
    m.fwd_variant = 100 + 10 * C; m.rev_variant = 100 + 10 * C + 3;
    m.bytes = 88.0; m.bytes_map = 88.0 + 8.0 / C; m.plain_bytes = 64.0; m.plain_bytes_map = 64.0 + 8.0 / C;
    m.adjoint_method = 14;
    return m;
}
const TapedModel kTapedColorWeighted[COLOR_MAX_C] = {taped_color_weighted(1), taped_color_weighted(2), taped_color_weighted(3),
                                                     taped_color_weighted(4)};

// The launch chains of a taped solve or of one of its sweeps: at most two (image groups on two streams)
// (channels > 1: the images of a chain are colour images, [lo, hi) the planes lo * channels ... hi * channels, so that no chain
// splits one)
void taped_chains(bpltv_t* h, const bpltv_params& p, const WeightedPlan& pl, ChainSolve* j, int channels = 1) {
    const int nimg = h->O / channels;
    j->nimg = nimg; j->niter = p.maxiter; j->T = pl.T;
    j->chains = plan_chains(p.reserved[1], pl.nTi * pl.nTj * nimg, h->ncu, nimg, 2);
    j->serial = (p.reserved[2] & 1) != 0; j->helper_thread = !(p.reserved[2] & 8);
}

// The tangent sweep of the channel-coupled model (color_tangent_tile_kernel): unrolled_jvp_common's
// launches with channels > 1.  The plan is the colour solve's; the first use raises the LDS its kernels may take.
int color_jvp_plan(bpltv_t* h, const bpltv_params& p, WeightedPlan* pl) {
    if (int prc = color_plan(h, p, PDHG_MAX_T, pl)) return prc;
    if (!h->color_jvp_ready) {
        HIPCHK(h, hipFuncSetAttribute((const void*)&color_tangent_tile_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_tangent_lds_bytes(2)));
        HIPCHK(h, hipFuncSetAttribute((const void*)&color_tangent_tile_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_tangent_lds_bytes(3)));
        HIPCHK(h, hipFuncSetAttribute((const void*)&color_tangent_tile_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)color_tangent_lds_bytes(4)));
        h->color_jvp_ready = true;
    }
    return BPLTV_OK;
}
// One launch of it: the caller has set the planes, alpha and the tangents (tv_tile_launch); s.lo, s.hi count colour images
void color_tangent_launch(bpltv_t* h, const WeightedPlan& pl, const double* tab, const LaunchStep& s, int channels, TvTileArgs& a) {
    a.f = h->d_f; a.tab = tab;
    a.it0 = s.it; a.nit = s.nit;
    a.M = h->M; a.N = h->N; a.halo = pl.T; a.first = s.first; a.img0 = s.lo;
    void (*kern)(TvTileArgs) = channels == 2 ? &color_tangent_tile_kernel<2> : (channels == 3 ? &color_tangent_tile_kernel<3> : &color_tangent_tile_kernel<4>);
    hipLaunchKernelGGL(kern, dim3(pl.nTi, pl.nTj, s.hi - s.lo), dim3(TV_R * TV_R), color_tangent_lds_bytes(channels), s.st, a);
}

// The end of a sweep through the iterations (the caller has put the last solve's statistics back): the time since ev[2] is
// its adjoint_ms, with its adjoint_method
int sweep_stats(bpltv_t* h, int method) {
    HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    h->st.adjoint_ms = ms;
    h->st.adjoint_method = method;
    return BPLTV_OK;
}

// Checkpointing (option "tape_checkpoint").  The effective spacing of a call of K iterations: 0 (the
// full tape), min(C, K), or (C = -1) the C that minimises nplanes * ceil(K / C) + tape_planes * C up to rounding:
// ceil(sqrt(nplanes * K / tape_planes)) in [1, K], in integers.
int tape_spacing(const TapedModel& m, int K, int C) {
    if (C == 0) return 0;
    if (C > 0) return std::min(C, K);
    const long long need = (long long)m.nplanes * K;
    long long c = (long long)std::sqrt((double)need / m.tape_planes);
    while (c * c * m.tape_planes < need) ++c;
    while (c > 1 && (c - 1) * (c - 1) * m.tape_planes >= need) --c;
    return (int)std::min<long long>(std::max<long long>(c, 1), K);
}
inline int tape_segments(int K, int C) { return (K + C - 1) / C; }

// The launches of the iterations [0, K) in segments of C, at most T per launch and none across a segment boundary:
// fn(it, nit, k0, e) for the iterations [it, it + nit) of the segment [k0, e).  stagger: the very first launch has T/2.
template <class F>
void segment_launches(int K, int C, int T, bool stagger, F fn) {
    int step = (stagger && T >= 2) ? T / 2 : T;
    for (int k0 = 0; k0 < K; k0 += C) {
        const int e = std::min(k0 + C, K);
        for (int it = k0; it < e; step = T) {
            const int nit = std::min(step, e - it);
            fn(it, nit, k0, e);
            it += nit;
        }
    }
}

// The taped solves on a single-device handle: bpltv_unrolled_denoise, bpltv_weighted_unrolled_denoise and
// bpltv_sumregs_unrolled_denoise with their _each and _device forms.  maxiter taped iterations on the dataset images, in the
// model's state sets, with d_alpha (each: O blocks, image k reads block k: upload_alpha); what the reverse sweep needs of
// every iteration and pixel goes onto d_tape_user, or (nullptr) onto the handle's own tape of the model, which grows here.
// The order is the contract: arguments, params, w, then the grown tape -- allocated before anything changes and installed only
// once upload_alpha has accepted the parameter -- and only then the handle's copy of w.
// With a checkpoint spacing C (option "tape_checkpoint") the same launches, cut at the segment boundaries, run the no-tape
// instantiation; the launch that ends segment s - 1 writes its state into slot s of the buffer instead of a state set, and
// the next one reads it from there (slot 0: x = f, y = 0).  The result ends in state set 0.
// !taped (bpltv_color_denoise, bpltv_color_weighted_denoise): the same launches of the no-tape instantiation and nothing else: no tape is written, grown or
// invalidated, and the checkpoint option does not apply.
int taped_denoise(bpltv_t* h, const TapedModel& m, const double* w, int wo, const double* alpha, bool dev, int am, int an,
                  const bpltv_params* pp, double* d_tape_user, double* u_out, bool each, bool taped = true) {
    const std::string name = taped ? std::string(m.denoise) + (each ? "_each" : "") + (dev ? "_device" : "")
                                   : std::string(m.kl ? "bpltv_kl_denoise" : m.l1 ? "bpltv_lone_denoise" : (m.weighted ? "bpltv_color_weighted_denoise" : "bpltv_color_denoise")) + (dev ? "_device" : "");
    const char* who = name.c_str();
    const int ch = m.channels ? m.channels : 1;
    const bool sr = m.slices == 3;
    Tape& tape = h->*m.tape;
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: bpltv_set_data has not been called", who);
    if (m.weighted) {
        if (!w) return set_err(h, BPLTV_E_ARG, "%s: w is a null pointer", who);
        if (wo != 1 && wo != h->O) return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, wo, h->O);
    }
    const bpltv_params p = resolve(pp, sr);
    if (int prc = unrolled_check_params(h, p, who)) return prc;
    WeightedPlan pl;
    if (int prc = m.plan(h, p, m.fwd_cap, &pl)) return prc;
    if (sr)
        if (int arc = sr_alloc(h)) return arc;
    const size_t nw = (size_t)wo * h->npx;
    double wmin = 0.0;
    int rc = m.weighted ? check_weight(h, who, w, dev, nw, &wmin) : (int)BPLTV_OK;
    if (rc) return rc;
    if (m.kl)
        if (int frc = check_dataset_nonneg(h, who)) return frc;
    const int K = p.maxiter, C = taped ? tape_spacing(m, K, h->opt.tape_checkpoint) : 0, np = m.nplanes;
    const size_t tot = h->tot;
    const size_t need = C ? (size_t)np * tape_segments(K, C) * tot : (size_t)m.tape_planes * K * tot;
    double* grown = nullptr;
    if (!d_tape_user && taped) {
        const hipError_t e = tape.grow(need, &grown);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return set_err(h, e == hipErrorOutOfMemory ? BPLTV_E_NOMEM : BPLTV_E_HIP, "%s: hipMalloc of the tape (%.1f MB) failed: %s", who,
                           need * sizeof(double) / 1e6, hipGetErrorString(e));
        }
    }
    if (m.weighted && !h->d_w) rc = alloc_all(h, {{(void**)&h->d_w, h->tot * sizeof(double)}}, "fidelity weight");
    if (rc == BPLTV_OK) {
        bpltv_params q = p;   // the planner's knobs and the forward variant mean nothing here: upload_alpha's precheck sees the defaults
        q.tile_iters = 0; q.reserved[0] = 0; q.reserved[1] = 0; q.reserved[2] = 0;
        rc = upload_alpha(h, alpha, dev, am, an, sr ? PRE_SR : PRE_TV, each ? h->O : 1, &q);
    }
    if (rc) {
        if (grown) (void)hipFree(grown);
        return rc;
    }
    tape.install(grown, need);
    if (!d_tape_user && taped) tape.valid = false;   // about to be overwritten
    if (m.weighted) {
        HIPCHK(h, hipMemcpyAsync(h->d_w, w, nw * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        h->w_wo = wo;
        h->w_min = wmin;
    }
    h->has_per_image = false;
    double* d_tab = nullptr;
    rc = get_table(h, p, &d_tab, m.L2, 0, m.flat() ? 0.0 : (m.weighted ? h->w_min : 1.0));
    if (rc) return rc;
    const bool amap = (h->last_am == h->M && h->last_an == h->N) && !(h->M == 1 && h->N == 1);
    h->st.tile_iters = pl.T; h->st.tiles = pl.nTi * pl.nTj * (h->O / ch); h->st.region_i = m.region; h->st.region_j = m.region; h->st.pdhg_variant = 0;
    double* const buffer = !taped ? nullptr : (d_tape_user ? d_tape_user : tape.d);   // the tape, or the checkpoints
    TapedFwd x{h, pl, d_tab, C ? nullptr : buffer, {}, h->d_alpha, h->last_am, h->last_an, h->alpha_istride, m.weighted ? h->d_w : nullptr, h->w_wo};
    x.channels = ch; x.l1 = m.l1; x.kl = m.kl;
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < np; ++c) x.S[s][c] = sr ? h->d_sr[s][c] : h->d_state[s][c];
    ChainSolve j;
    j.model = m.graphs; j.nplanes = np; j.state0 = sr ? h->d_sr[0] : h->d_state[0];
    taped_chains(h, p, pl, &j, ch);
    j.bytes_per_px_iter = (C || !taped) ? (amap ? m.plain_bytes_map : m.plain_bytes) : (amap ? m.bytes_map : m.bytes);
    // (istride: a per-image solve uploads into d_alpha like a shared one, and must not replay its graph, nor the reverse)
    j.key = GraphKey{K, pl.T, m.fwd_variant + (taped ? 0 : 2), h->last_am, h->last_an, j.chains, 0.0, 0.0, 0.0, 0, 0, 0, (const void*)buffer, (const void*)d_tab, 0,
                     (const void*)h->d_alpha, m.weighted ? 0 : h->alpha_istride, m.weighted ? h->w_wo : 0, C, nullptr, 0};
    if (!C) {
        j.enqueue = launch_loop(pl.T, [&](const LaunchStep& s) { m.launch_fwd(x, s); });
    } else {
        const int T = pl.T;
        auto to_slot = [K](int nit_end, int e) { return nit_end == e && e < K; };   // the launch ends a segment that has a successor
        // slot 0, the state every solve starts from, is layout only: it keeps the slots uniform and a caller's buffer fully
        // defined, but neither the solve nor the sweep reads it -- segment 0 starts with first = 1, as a full-tape solve does
        j.begin = [&]() {
            HIPCHK(h, hipMemcpyAsync(buffer, h->d_f, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemsetAsync(buffer + tot, 0, (size_t)(np - 1) * tot * sizeof(double), h->stream));
            return (int)BPLTV_OK;
        };
        j.result_set = 0;
        j.chain_launches = [=](bool stagger) {
            int n = 0;
            segment_launches(K, C, T, stagger, [&](int, int, int, int) { ++n; });
            return n;
        };
        // the launches that write a state set alternate so that the last one writes set 0; one that reads a set reads the one
        // written last, which is the other one
        j.enqueue = [&, K, C, T, np, tot, buffer, to_slot](hipStream_t st, int, int, int, int lo, int hi, bool stagger) {
            int W = 0, wr = 0, cur = 0;
            segment_launches(K, C, T, stagger, [&](int it, int nit, int, int e) { W += to_slot(it + nit, e) ? 0 : 1; });
            segment_launches(K, C, T, stagger, [&](int it, int nit, int k0, int e) {
                LaunchStep ls{st, it, nit, cur, cur, (it == 0) ? 1 : 0, lo, hi};
                if (it == k0 && it > 0) ls.ckin = buffer + (size_t)(k0 / C) * np * tot;
                if (to_slot(it + nit, e)) {
                    ls.ckout = buffer + (size_t)(e / C) * np * tot;
                } else {
                    ls.nxt = (W - 1 - wr) % 2;
                    ++wr;
                    cur = ls.nxt;
                }
                m.launch_fwd(x, ls);
            });
            return 0;
        };
    }
    int buf = 0;
    rc = run_chains(h, p, j, &buf);
    if (rc) return rc;
    h->st.algorithmic_bytes *= ch;   // (the driver counted colour images)
    if (sr) {   // committed like bpltv_sumregs_denoise's
        h->sr_result_buf = buf;
        h->sr_has_result = true;
    } else {
        h->result_buf = buf;
        h->has_result = true;
    }
    h->last_is_sr = sr;
    h->last_weighted = m.weighted;
    h->last_channels = m.channels;
    h->last_l1 = m.l1;
    h->last_kl = m.kl;
    if (!d_tape_user && taped) {
        tape.record(p, am, an, each, m.weighted ? wo : 0, m.flat() ? 0.0 : wmin, C);
        tape.channels = m.channels;
    }
    if (u_out) {
        HIPCHK(h, hipMemcpyAsync(u_out, sr ? h->d_sr[buf][0] : h->d_state[buf][0], h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// The per-pixel, per-image parameter gradient d_ga ([slices][O][M*N]) into d_grad_alpha, slice by slice in a fixed order
// without atomics.  Shared parameter: slice r is the sum of ga_r over the images in image order, then per patch
// (calc_adjoint) or over everything.  each: O blocks of [slices][am*an], block k image k's own -- the plane as it is for a map,
// image k's patch sums otherwise.
int reduce_grad_alpha(bpltv_t* h, const double* d_ga, int slices, int am, int an, bool each, double* d_grad_alpha) {
    const int M = h->M, N = h->N, O = h->O, sl = am * an;
    const size_t tot = h->tot, npx = h->npx;
    const bool amap = am == M && an == N && !(M == 1 && N == 1);
    for (int r = 0; r < slices; ++r) {
        const double* ga_r = d_ga + (size_t)r * tot;
        if (each && amap && slices == 1) {
            HIPCHK(h, hipMemcpyAsync(d_grad_alpha, ga_r, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        } else if (each && amap) {   // the plane of the slice, image by image
            HIPCHK(h, hipMemcpy2DAsync(d_grad_alpha + (size_t)r * npx, slices * npx * sizeof(double), ga_r, npx * sizeof(double), npx * sizeof(double), O,
                                       hipMemcpyDeviceToDevice, h->stream));
        } else if (each) {
            hipLaunchKernelGGL(patch_sum_kernel, dim3(sl, O), dim3(256), 0, h->stream, ga_r, M, N, O, am, an, 1, slices * sl, d_grad_alpha + (size_t)r * sl);
        } else if (amap) {
            hipLaunchKernelGGL(map_sum_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, ga_r, npx, O, d_grad_alpha + (size_t)r * npx);
        } else {
            double* red = h->d_red + (size_t)r * sl * O;
            hipLaunchKernelGGL(patch_sum_kernel, dim3(sl, O), dim3(256), 0, h->stream, ga_r, M, N, O, am, an, O, 1, red);
            hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, h->stream, red, O, sl, 1.0, d_grad_alpha + (size_t)r * sl, (double*)nullptr);
        }
    }
    return BPLTV_OK;
}

// The reverse sweeps on a single-device handle: bpltv_unrolled_vjp, bpltv_weighted_unrolled_vjp and bpltv_sumregs_unrolled_vjp
// with their _each and _device forms.  d_gu and the outputs live in HBM; alpha (slices*am*an doubles, or O such blocks: each)
// and the weighted model's w (every entry >= 0) on the host or (dev) in HBM; d_tape_user or the handle's tape of the model,
// which must have been recorded by this call's solve.  Parameter and weight are staged apart (stage_param) and the sweep runs
// in planes of its own, so the last solve stays untouched; the solve statistics are put back after the shared driver has run
// the sweep.  The step table is the solve's (weighted: gamma = min w), held fixed.  d_grad_w (weighted only) needs the resident f.
// With a checkpoint spacing C (option "tape_checkpoint") the buffer holds the checkpoints of that spacing, and the sweep runs
// segment by segment, last to first, all in one launch sequence: the taping kernel re-runs the segment's iterations from its
// checkpoint on the staged parameter (and weight) and the resident f, in state planes of its own, into the handle's segment
// tape (d_seg); the reverse kernel then undoes them, carrying its planes on from the segment before.  The checkpoints are
// only read.  An out-of-phase chain starts its first recompute launch at half depth, as the solve's does.
int taped_vjp(bpltv_t* h, const TapedModel& m, const double* d_tape_user, const double* w, int wo, const double* alpha, bool dev, int am,
              int an, const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha, double* d_grad_w, bool each) {
    const std::string name = std::string(m.vjp) + (each ? "_each" : "");
    const char* who = name.c_str();
    const bool sr = m.slices == 3;
    const Tape& tape = h->*m.tape;
    if (!alpha || !d_gu || (m.weighted && !w)) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (!d_grad_f && !d_grad_alpha && !d_grad_w) return set_err(h, BPLTV_E_ARG, "%s: %s outputs are NULL", who, m.weighted ? "all three" : "both");
    if (m.weighted && wo != 1 && wo != h->O)
        return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, wo, h->O);
    const bpltv_params p0 = resolve(pp, sr);
    if (int prc = unrolled_check_params(h, p0, who)) return prc;
    if (d_grad_w && !h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: grad_w reads the resident f: bpltv_set_data has not been called", who);
    if (m.l1 && !h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: the L1 sweep reads the resident f: bpltv_set_data has not been called", who);
    if (m.kl && !h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: the KL sweep reads the resident f: bpltv_set_data has not been called", who);
    const int K = p0.maxiter, C = tape_spacing(m, K, h->opt.tape_checkpoint);
    if (C && !h->has_data)
        return set_err(h, BPLTV_E_NODATA, "%s: a checkpointed sweep recomputes on the resident f: bpltv_set_data has not been called", who);
    if (!d_tape_user) {
        if (!tape.valid) return set_err(h, BPLTV_E_NODATA, "%s: the handle holds no %stape (%s has not run)", who, m.tape_kind, m.denoise);
        if (!tape.made_with(p0, am, an, m.weighted ? wo : 0))
            return set_err(h, BPLTV_E_ARG, "%s: the handle's tape was recorded with maxiter = %d, a %dx%d parameter, wo = %d and other steps than this call's (%d, %dx%d, wo = %d)",
                           who, tape.maxiter, tape.am, tape.an, tape.wo, p0.maxiter, am, an, m.weighted ? wo : 0);
        if (tape.each != each)
            return set_err(h, BPLTV_E_ARG, "%s: the handle's tape was recorded with one %s (%s%s)", who,
                           tape.each ? "parameter block per image" : "shared parameter", m.denoise, tape.each ? "_each" : "");
        if (tape.channels != m.channels)
            return set_err(h, BPLTV_E_ARG, "%s: the handle's %stape was recorded with channels = %d, this call has %d", who, m.tape_kind, tape.channels, m.channels);
        if (tape.spacing != C)
            return set_err(h, BPLTV_E_ARG, "%s: the handle's %stape was recorded with checkpoint spacing %d (0: the full tape), option tape_checkpoint gives %d",
                           who, m.tape_kind, tape.spacing, C);
    }
    WeightedPlan pl, plf{};
    if (int prc = m.plan(h, p0, m.rev_cap, &pl)) return prc;
    if (C)
        if (int prc = m.plan(h, p0, m.fwd_cap, &plf)) return prc;
    const size_t tot = h->tot, npx = h->npx;
    const int np = m.nplanes;
    double*& d_ws = h->*m.sweep;
    if (!d_ws)
        if (int arc = alloc_all(h, {{(void**)&d_ws, (2 * np + 2 + m.slices) * tot * sizeof(double)}}, m.sweep_name)) return arc;
    if (d_grad_w && !h->d_unr_gw)
        if (int arc = alloc_all(h, {{(void**)&h->d_unr_gw, tot * sizeof(double)}}, "reverse sweep (weight gradient)")) return arc;
    bpltv_params p;
    GradCtx g;
    if (int rc = stage_param(h, who, alpha, dev, am, an, m.slices, each, 0, &p0, m.weighted ? w : nullptr, m.weighted ? wo : 1,
                             {{d_gu, tot, "cotangent gu"}}, &p, &g, false))
        return rc;
    if (m.weighted && !m.flat() && !d_tape_user && tape.gamma != g.w_min)
        return set_err(h, BPLTV_E_ARG, "%s: the handle's tape was recorded with gamma = min w = %g, this call's w has %g", who, tape.gamma, g.w_min);
    const bool amap = am == h->M && an == h->N && !(h->M == 1 && h->N == 1);
    if (d_grad_alpha && !amap && !each)
        if (int rc = ensure(h, &h->d_red, &h->red_cap, (size_t)m.slices * am * an * h->O)) return rc;
    h->has_per_image = false;
    double* d_tab = nullptr;
    if (int rc = get_table(h, p, &d_tab, m.L2, 0, m.flat() ? 0.0 : (m.weighted ? g.w_min : 1.0))) return rc;
    const size_t seg_tape = (size_t)m.tape_planes * C * tot, seg_need = seg_tape + (size_t)2 * np * tot;
    // grown after the last rejection, so that a rejected call never moves it (and orphans the graphs keyed by it); the new
    // buffer first: a failed allocation leaves the handle as it was
    if (C && h->seg_cap < seg_need) {
        double* d_new = nullptr;
        const hipError_t e = hipMalloc((void**)&d_new, seg_need * sizeof(double));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return set_err(h, e == hipErrorOutOfMemory ? BPLTV_E_NOMEM : BPLTV_E_HIP, "%s: hipMalloc of the segment tape (%.1f MB) failed: %s", who,
                           seg_need * sizeof(double) / 1e6, hipGetErrorString(e));
        }
        if (h->d_seg) (void)hipFree(h->d_seg);
        h->d_seg = d_new;
        h->seg_cap = seg_need;
    }
    TapedRev x{h, pl, d_tab, d_tape_user ? d_tape_user : tape.d, &g, {}, d_ws + (size_t)2 * np * tot, d_ws + (size_t)(2 * np + 1) * tot,
               d_ws + (size_t)(2 * np + 1 + m.slices) * tot, d_grad_w ? h->d_unr_gw : nullptr, p.maxiter};
    x.channels = m.channels ? m.channels : 1; x.l1 = m.l1; x.kl = m.kl;
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < np; ++c) x.S[s][c] = d_ws + (size_t)(np * s + c) * tot;
    const bpltv_stats_t kept = h->st;
    HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
    HIPCHK(h, hipMemcpyAsync(x.g0, d_gu, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    ChainSolve j;
    j.model = m.graphs; j.nplanes = np; j.state0 = x.S[0];
    taped_chains(h, p, pl, &j, x.channels);
    j.bytes_per_px_iter = 0.0;   // (the driver's solve statistics are not this call's: `kept` goes back below)
    j.key = GraphKey{p.maxiter, pl.T, m.rev_variant + (x.gw ? 1 : 0), am, an, j.chains, 0.0, 0.0, 0.0, 0, 0, 0, (const void*)x.tape, (const void*)d_tab, 0,
                     (const void*)g.alpha, m.weighted ? 0 : g.astride, m.weighted ? wo : 0, C, C ? (const void*)h->d_seg : nullptr, C ? plf.T : 0};
    TapedFwd xf{h, plf, d_tab, h->d_seg, {}, g.alpha, g.am, g.an, g.astride, g.w, g.wo};   // the recompute of a segment
    xf.channels = x.channels; xf.l1 = m.l1; xf.kl = m.kl;
    if (!C) {
        j.enqueue = launch_loop(pl.T, [&](const LaunchStep& s) { m.launch_rev(x, s); });
    } else {
        const int Tr = pl.T, Tf = plf.T, nseg = tape_segments(K, C);
        const double* const ck = x.tape;   // the checkpoints
        x.tape = h->d_seg;                 // what the reverse launches read
        for (int s = 0; s < 2; ++s)
            for (int c = 0; c < np; ++c) xf.S[s][c] = h->d_seg + seg_tape + (size_t)(np * s + c) * tot;
        auto rev_launches = [=](int len) { return (len + Tr - 1) / Tr; };
        int W = 0, F = 0;   // reverse / recompute launches of a chain
        for (int k0 = 0; k0 < K; k0 += C) {
            W += rev_launches(std::min(C, K - k0));
            F += (std::min(C, K - k0) + Tf - 1) / Tf;
        }
        // an out-of-phase chain: the first recompute launch (of the last segment) has Tf / 2 iterations
        const int last_len = K - (nseg - 1) * C, half = Tf / 2;
        const int F_oop = F - (last_len + Tf - 1) / Tf + 1 + (last_len > half && half > 0 ? (last_len - half + Tf - 1) / Tf : 0);
        j.result_set = 0;
        j.chain_launches = [=](bool stagger) { return W + ((stagger && half > 0) ? F_oop : F); };
        // the reverse launches alternate between the sweep's two sets so that the last one writes set 0
        j.enqueue = [&, K, C, Tr, Tf, nseg, np, tot, ck, W](hipStream_t st, int, int, int, int lo, int hi, bool stagger) {
            int wr = 0, rcur = 0;
            int step = (stagger && Tf >= 2) ? Tf / 2 : Tf;
            for (int sg = nseg - 1; sg >= 0; --sg) {
                const int k0 = sg * C, e = std::min(k0 + C, K);
                int fcur = 0;
                for (int it = k0, nit = 0; it < e; it += nit, step = Tf) {
                    nit = std::min(step, e - it);
                    LaunchStep ls{st, it, nit, fcur, 1 - fcur, (it == 0) ? 1 : 0, lo, hi};
                    ls.tk0 = k0;
                    if (it == k0 && it > 0) ls.ckin = ck + (size_t)sg * np * tot;
                    m.launch_fwd(xf, ls);
                    fcur = 1 - fcur;
                }
                for (int khi = e - 1; khi >= k0; khi -= Tr) {
                    LaunchStep ls{st, K - 1 - khi, std::min(Tr, khi - k0 + 1), rcur, (W - 1 - wr) % 2, (wr == 0) ? 1 : 0, lo, hi};
                    ls.tk0 = k0;
                    m.launch_rev(x, ls);
                    rcur = ls.nxt;
                    ++wr;
                }
            }
            return 0;
        };
    }
    int buf = 0;
    const int rc = run_chains(h, p, j, &buf);
    h->st = kept;
    if (rc) return rc;
    if (d_grad_f)
        hipLaunchKernelGGL(unrolled_gradf_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, x.gf, x.S[buf][0], tot, d_grad_f);
    if (d_grad_alpha)
        if (int rrc = reduce_grad_alpha(h, x.ga, m.slices, am, an, each, d_grad_alpha)) return rrc;
    if (d_grad_w && wo > 1) {   // per image: the plane as it is; one plane: the sum over the images in image order
        HIPCHK(h, hipMemcpyAsync(d_grad_w, x.gw, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    } else if (d_grad_w) {
        hipLaunchKernelGGL(map_sum_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, x.gw, npx, h->O, d_grad_w);
    }
    HIPCHK(h, hipGetLastError());
    if (int src = sweep_stats(h, m.adjoint_method)) return src;
    if (m.tv_stats) {
        h->st.reg_gradient_used = 0;
        h->st.adjoint_attempts = 1;
        h->st.adjoint_chunks = 1;
        h->st.hb_sync = 0;
        h->st.kappa_used = 0.0;
        h->st.adjoint_residual = 0.0;
        h->st.adjoint_residual_raw = 0.0;
    }
    return BPLTV_OK;
}

// bpltv_unrolled_jvp(_device), bpltv_weighted_unrolled_jvp(_device) and the two Gauss-Newton calls on a single-device handle
// (tv_tile_kernels.hpp; DESIGN.md sections 4.7 and 4.11): ndir tangent sweeps, one after
// the other, each the same launch sequence (direction d of a call is bitwise the call with that direction alone).  The tangents
// d_df / d_dalpha (and the weighted model's d_dw; any may be nullptr: a zero tangent) and d_du live in HBM, direction-major; alpha
// (and w) on the host or (dev) in HBM.  Every sweep runs in planes of the handle's own -- d_ujv = [2 sets x (x, y1, y2, dx, dy1,
// dy2) | df | dalpha], weighted: d_wjv = [2 sets | df | dalpha | w | dw | 8 check words] -- on the staged parameter (stage_param),
// with the direction's tangents copied into the workspace first, so that no captured graph holds a caller's address and the
// last solve, the tapes and the solve statistics stay as they were.
// d_u (nullable): receives the primal result, bpltv_denoise's (bpltv_weighted_denoise's) u.  *x_res (nullable): the workspace
// plane that holds it.
// each (bpltv_unrolled_jvp_each(_device)): alpha holds O blocks and d_dalpha ndir x O blocks (direction, then image); image k
// reads block k of both.
// W (nullable: the TV model): the weighted model's w (wo planes, every entry >= 0) and d_dw (ndir x wo planes).  The step table
// has gamma = min w, held fixed.  W->data (bpltv_lone_unrolled_jvp, bpltv_kl_unrolled_jvp and their Gauss-Newton calls; DESIGN.md
// section 4.20): the TV-L1 or the TV-KL data term in place of the quadratic one -- the same workspace and launches with the
// model's tangent instantiation, the step table of gamma = 0 (TapedModel::flat()) and graph variants of its own; TV-KL looks at
// the dataset first (check_dataset_nonneg).
// channels (bpltv_color_unrolled_jvp(_device), bpltv_color_unrolled_gauss_newton): the planes of a colour
// image, 1 ... 4, dividing O; 0: the TV or weighted call.  The same driver with color_plan's plan, launch chains that count
// colour images, color_tangent_tile_kernel and graphs of their own under MODEL_COLOR; channels = 1 runs the TV tangent kernel.
enum JvpData { JVP_QUADRATIC = 0, JVP_L1 = 1, JVP_KL = 2 };   // the data term of a weighted sweep
struct JvpWeight {
    const double* w;
    int wo;
    const double* dw;   // HBM in unrolled_jvp_common; the host array in unrolled_jvp_host
    int data = JVP_QUADRATIC;
};
// The tangent instantiation of tv_tile_kernel of a model, with its dynamic LDS (two sets of planes: above the default limit)
// allowed: once per instantiation and handle (the attribute is the device's), whoever allocated the workspace the sweeps share
int tangent_kernel_ready(bpltv_t* h, bool weighted, int data) {
    const int k = !weighted ? 0 : 1 + data;
    if (h->tangent_lds_set[k]) return BPLTV_OK;
    const void* fn = k == 0   ? reinterpret_cast<const void*>(&tv_tile_kernel<false, false, true>)
                     : k == 1 ? reinterpret_cast<const void*>(&tv_tile_kernel<true, false, true>)
                     : k == 2 ? reinterpret_cast<const void*>(&tv_tile_kernel<true, false, true, true>)
                              : reinterpret_cast<const void*>(&tv_tile_kernel<true, false, true, false, true>);
    HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tv_tangent_lds_bytes()));
    h->tangent_lds_set[k] = true;
    return BPLTV_OK;
}
int unrolled_jvp_common(bpltv_t* h, const char* who, const double* alpha, bool dev, int am, int an, const bpltv_params* pp, int ndir,
                        const double* d_df, const double* d_dalpha, double* d_du, double* d_u, const double** x_res, bool each = false,
                        const JvpWeight* W = nullptr, int channels = 0) {
    const double* d_dw = W ? W->dw : nullptr;
    const int data = W ? W->data : (int)JVP_QUADRATIC;
    const bool flat = data != JVP_QUADRATIC;   // TapedModel::flat(): no strong convexity, gamma = 0
    if (!alpha || !d_du || (W && !W->w)) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (ndir < 1) return set_err(h, BPLTV_E_ARG, "%s: ndir = %d (at least one direction)", who, ndir);
    if (!d_df && !d_dalpha && !d_dw) return set_err(h, BPLTV_E_ARG, "%s: %s tangents are NULL", who, W ? "all three" : "both");
    if (W && W->wo != 1 && W->wo != h->O)
        return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, W->wo, h->O);
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: bpltv_set_data has not been called", who);
    const bpltv_params p0 = resolve(pp);
    if (int prc = unrolled_check_params(h, p0, who)) return prc;
    WeightedPlan pl;
    if (int prc = channels > 1 ? color_jvp_plan(h, p0, &pl) : unrolled_plan(h, p0, PDHG_MAX_T, &pl)) return prc;
    if (data == JVP_KL)   // (memoised with the dataset; before anything of the handle changes)
        if (int frc = check_dataset_nonneg(h, who)) return frc;
    const size_t tot = h->tot, nw = W ? (size_t)W->wo * h->npx : 0;
    double*& d_ws = W ? h->d_wjv : h->d_ujv;   // (the three weighted models share d_wjv)
    if (!d_ws)
        if (int arc = alloc_all(h, {{(void**)&d_ws, ((W ? 16 : 14) * tot + (W ? 8 : 0)) * sizeof(double)}}, W ? "weighted tangent sweep" : "tangent sweep"))
            return arc;
    if (channels <= 1)
        if (int lrc = tangent_kernel_ready(h, W != nullptr, data)) return lrc;
    const size_t P = (size_t)am * an * (each ? h->O : 1);   // (stage_param checks the shape before it reads anything)
    if (d_dw) {   // the third tangent: a read-back of its own (stage_param's takes two), into the workspace's check words
        int failed = -1;
        double unused = 0.0;
        if (int rc = check_device_arrays(h, reinterpret_cast<unsigned long long*>(d_ws + 16 * tot), {nullptr, 0}, {{d_dw, (size_t)ndir * nw, "tangent dw"}}, &unused, &failed))
            return rc;
        if (failed > 0) return set_err(h, BPLTV_E_ARG, "%s: the tangent dw must be finite", who);
    }
    bpltv_params p;
    GradCtx g;
    if (int rc = stage_param(h, who, alpha, dev, am, an, 1, each, 0, pp, W ? W->w : nullptr, W ? W->wo : 1,
                             {{d_df, (size_t)ndir * tot, "tangent df"}, {d_dalpha, (size_t)ndir * P, "tangent dalpha"}}, &p, &g, false))
        return rc;
    double* d_tab = nullptr;
    if (int rc = get_table(h, p, &d_tab, 8.0, 0, flat ? 0.0 : (W ? g.w_min : 1.0))) return rc;
    const int T = pl.T, K = p.maxiter;
    double* S[2][6];
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 6; ++c) S[s][c] = d_ws + (size_t)(6 * s + c) * tot;
    double *d_dfc = d_ws + 12 * tot, *d_dac = d_ws + 13 * tot;   // (a parameter has at most M*N <= tot entries)
    double *d_wc = W ? d_ws + 14 * tot : nullptr, *d_dwc = W ? d_ws + 15 * tot : nullptr;
    if (W) HIPCHK(h, hipMemcpyAsync(d_wc, g.w, nw * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    const bpltv_stats_t kept = h->st;
    ChainSolve j;
    j.model = channels > 1 ? MODEL_COLOR : MODEL_UN; j.nplanes = 6; j.state0 = S[0];
    taped_chains(h, p, pl, &j, channels ? channels : 1);
    j.bytes_per_px_iter = 0.0;   // (the driver's solve statistics are not this call's: `kept` goes back below)
    // variant 2 ... 5: a tangent sweep, by which tangents it reads (0 = taped solve, 1 = reverse sweep); 9 ... 16: a weighted one;
    // 41 ... 47: a TV-L1 one; 51 ... 57: a TV-KL one (the three share d_wjv, and with min w = 0 the step table as well);
    // MODEL_COLOR: 10 * channels + 3 + tangents (+ 0 ... 2 are the model's solves and its reverse sweep)
    const int tangents = (d_df ? 1 : 0) + (d_dalpha ? 2 : 0) + (d_dw ? 4 : 0);
    j.key = GraphKey{K, T, (channels > 1 ? 10 * channels + 3 : (data == JVP_L1 ? 40 : data == JVP_KL ? 50 : (W ? 9 : 2))) + tangents, am, an, j.chains, 0.0, 0.0, 0.0, 0, 0, 0, (const void*)d_ws,
                     (const void*)d_tab, 0, (const void*)g.alpha, g.astride, W ? W->wo : 0};
    j.enqueue = launch_loop(T, [&](const LaunchStep& s) {
        TvTileArgs a{};
        for (int c = 0; c < 6; ++c) { a.in[c] = S[s.cur][c]; a.out[c] = S[s.nxt][c]; }
        a.w = d_wc; a.wstride = (W && W->wo > 1) ? h->npx : 0;
        a.alpha = g.alpha; a.am = am; a.an = an; a.istride = g.astride;
        a.df = d_df ? d_dfc : nullptr; a.dw = d_dw ? d_dwc : nullptr; a.dalpha = d_dalpha ? d_dac : nullptr;
        if (channels > 1) color_tangent_launch(h, pl, d_tab, s, channels, a);
        else tv_tile_launch(h, pl, d_tab, s, W != nullptr, true, a, data == JVP_L1, data == JVP_KL);
    });
    int rc = hipEventRecord(h->ev[2], h->stream) == hipSuccess ? (int)BPLTV_OK : set_err(h, BPLTV_E_HIP, "%s: hipEventRecord failed", who);
    int buf = 0;
    for (int d = 0; d < ndir && rc == BPLTV_OK; ++d) {
        hipError_t e = hipSuccess;
        if (d_df) e = hipMemcpyAsync(d_dfc, d_df + (size_t)d * tot, tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (d_dalpha && e == hipSuccess) e = hipMemcpyAsync(d_dac, d_dalpha + (size_t)d * P, P * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (d_dw && e == hipSuccess) e = hipMemcpyAsync(d_dwc, d_dw + (size_t)d * nw, nw * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) { rc = set_err(h, BPLTV_E_HIP, "%s: copy of the tangents failed: %s", who, hipGetErrorString(e)); break; }
        rc = run_chains(h, p, j, &buf);
        if (rc) break;
        e = hipMemcpyAsync(d_du + (size_t)d * tot, S[buf][3], tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) rc = set_err(h, BPLTV_E_HIP, "%s: copy of du failed: %s", who, hipGetErrorString(e));
    }
    h->st = kept;
    if (rc) return rc;
    if (d_u) HIPCHK(h, hipMemcpyAsync(d_u, S[buf][0], tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (int src = sweep_stats(h, channels ? 13 : (data == JVP_L1 ? 17 : data == JVP_KL ? 18 : (W ? 11 : 8)))) return src;
    if (x_res) *x_res = S[buf][0];
    return BPLTV_OK;
}

// n entries of a host tangent array (nullable), all finite
int check_tangent_host(bpltv_t* h, const char* who, const char* name, const double* a, size_t n) {
    if (!a) return BPLTV_OK;
    for (size_t e = 0; e < n; ++e)
        if (!std::isfinite(a[e])) return set_err(h, BPLTV_E_ARG, "%s: the %s must be finite (entry %zu = %g)", who, name, e, a[e]);
    return BPLTV_OK;
}

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================
#pragma GCC visibility push(default)
extern "C" {

int bpltv_version(void) { return BPLTV_VERSION; }

int bpltv_default_params(bpltv_params* p) {
    if (!p) return BPLTV_E_ARG;
    std::memset(p, 0, sizeof(*p));
    p->rho = 0.0;            // /root/reference/src/TVLearningFunctionVec.jl:34
    p->tau0 = 5.0;           // :36
    p->sigma0 = 0.99 / 5;    // :37
    p->accel = 1;            // :38
    p->maxiter = 5000;       // :40
    p->delta_t = 1e-6;       // :14
    p->check_every = 0;
    p->gap_tol = 0.0;
    p->tile_iters = 0;
    p->use_graph = 1;
    p->kappa_cap = 0.0;
    p->refine = -1;
    return BPLTV_OK;
}

int bpltv_create(bpltv_t** out, int M, int N, int O, int device, int dtype) {
    if (!out) return BPLTV_E_ARG;
    *out = nullptr;
    if (M < 1 || N < 1 || O < 1 || (dtype != 64 && dtype != 32)) return BPLTV_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BPLTV_E_HIP;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return BPLTV_E_HIP;
    }
    if (device >= ndev) return BPLTV_E_ARG;
    bpltv_t* h = new (std::nothrow) bpltv_handle();
    if (!h) return BPLTV_E_NOMEM;
    h->M = M; h->N = N; h->O = O; h->device = device; h->dtype = dtype;
    h->npx = (size_t)M * N;
    h->tot = h->npx * O;
    std::memset(&h->st, 0, sizeof(h->st));
    h->st.M = M; h->st.N = N; h->st.O = O; h->st.device = device;
    h->st.last_gap = -1.0;
    h->st.ngpus = 1;
    *out = h;  // returned even on failure below so that bpltv_last_error works; caller destroys
    HIPCHK(h, hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->ncu = prop.multiProcessorCount;
        h->st.ncu = h->ncu;
    }
    HIPCHK(h, device_streams_acquire(device, &h->stream));
    for (auto& e : h->ev) HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
    HIPCHK(h, hipMalloc((void**)&h->d_phase, 64));
    HIPCHK(h, hipMemset(h->d_phase, 0, 64));
    HIPCHK(h, hipMalloc((void**)&h->d_ubar, h->tot * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->d_f, h->tot * sizeof(double)));
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) HIPCHK(h, hipMalloc((void**)&h->d_state[s][c], h->tot * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->d_perimg, (size_t)O * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->d_scalar, 4 * sizeof(double)));
    // LDS above 64 KB needs the opt-in attribute
    for (const Variant& V : kVariants) {
        if (V.lds > 64 * 1024)
            HIPCHK(h, hipFuncSetAttribute(V.func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)V.lds));
        if (dtype == 32 && V.lds32 > 64 * 1024)
            HIPCHK(h, hipFuncSetAttribute(V.func32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)V.lds32));
        if (V.func_1d && V.lds > 64 * 1024)
            HIPCHK(h, hipFuncSetAttribute(V.func_1d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)V.lds));
        if (V.func32_1d && dtype == 32 && V.lds32 > 64 * 1024)
            HIPCHK(h, hipFuncSetAttribute(V.func32_1d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)V.lds32));
    }
    return BPLTV_OK;
}

int bpltv_create_sharded(bpltv_t** out, int M, int N, int O, const int* devices, int nshards, int dtype) {
    return multi_create(out, M, N, O, devices, nshards, dtype);
}

int bpltv_create_multi(bpltv_t** out, int M, int N, int O, int ngpus, int dtype) {
    if (!out) return BPLTV_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BPLTV_E_HIP;
    if (ngpus == 0) ngpus = ndev;   // all visible devices
    if (ngpus < 0 || ngpus > ndev) return BPLTV_E_ARG;
    std::vector<int> devs(ngpus);
    for (int k = 0; k < ngpus; ++k) devs[k] = k;
    return multi_create(out, M, N, O, devs.data(), ngpus, dtype);
}

int bpltv_destroy(bpltv_t* h) {
    if (!h) return BPLTV_OK;
    if (h->multi) {
        multi_free(h);
        delete h;
        return BPLTV_OK;
    }
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->launcher.reset();   // joins the launcher thread (idle: every call waits for its job)
    drop_graphs(h, DROP_ALL);
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (auto ce : h->chain_events) (void)hipEventDestroy(ce);   // (the chain streams belong to the device: device_streams_release below)
    if (h->capture_stream) (void)hipStreamDestroy(h->capture_stream);
    if (h->d_phase) (void)hipFree(h->d_phase);
    for (auto& kv : h->tabs) (void)hipFree(kv.second);
    for (auto& kv : h->tabs32) (void)hipFree(kv.second);
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c)
            if (h->f32_state[s][c]) (void)hipFree(h->f32_state[s][c]);
    if (h->f32_f) (void)hipFree(h->f32_f);
    if (h->f32_alpha) (void)hipFree(h->f32_alpha);
    if (h->f32_sweep_alpha) (void)hipFree(h->f32_sweep_alpha);
    void* ptrs[] = {h->d_ubar, h->d_f, h->d_alpha, h->d_sweep_alpha, h->d_partial, h->d_red, h->d_perimg, h->d_scalar, h->d_coef,
                    h->d_band4, h->d_bcr, h->d_L, h->d_invF, h->d_invB, h->d_L1, h->d_dump, h->d_Lm, h->d_spill, h->d_p, h->d_r, h->d_gpix, h->d_resn, h->d_fail, h->d_u2, h->d_ubar2,
                    h->d_gf2, h->d_vjp, h->d_jvp, h->d_jres, h->d_w, h->d_wst, h->d_unr, h->d_ujv, h->d_wjv, h->d_unr_gw, h->d_srunr, h->d_seg};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (Tape* t : {&h->tape, &h->wtape, &h->srtape, &h->ctape, &h->cwtape, &h->l1tape, &h->kltape}) t->release();
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) {
            if (h->d_state[s][c]) (void)hipFree(h->d_state[s][c]);
            if (h->d_sweep[s][c]) (void)hipFree(h->d_sweep[s][c]);
        }
    if (h->d_sweep_cost) (void)hipFree(h->d_sweep_cost);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    h->hb.release();
    h->nd.release();
    h->nd_sr.release();
    h->nd_sr_lu.release();
    h->hb_sr.release();
    h->lu_sr.release();
    if (h->d_srdiagU) (void)hipFree(h->d_srdiagU);
    for (void* q : {(void*)h->d_srcoef, (void*)h->d_srdiag, (void*)h->d_srw, (void*)h->d_srgpix, (void*)h->d_srsweep_alpha,
                    (void*)h->d_srsweep_cost})
        if (q) (void)hipFree(q);
    for (int s2 = 0; s2 < 2; ++s2)
        for (int c = 0; c < 7; ++c) {
            if (h->d_sr[s2][c]) (void)hipFree(h->d_sr[s2][c]);
            if (h->d_srsweep[s2][c]) (void)hipFree(h->d_srsweep[s2][c]);
        }
    if (h->stream) device_streams_release(h->device);
    delete h;
    return BPLTV_OK;
}

static int set_data_impl(bpltv_t* h, const double* ubar, const double* f, hipMemcpyKind kind) {
    if (!h) return BPLTV_E_ARG;
    if (!ubar || !f) return set_err(h, BPLTV_E_ARG, "set_data: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar, ubar, h->tot * sizeof(double), kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_f, f, h->tot * sizeof(double), kind, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->has_data = true;
    h->has_result = false;
    h->f32_f_valid = false;
    h->f_nonneg = -1;
    for (Tape* t : {&h->tape, &h->wtape, &h->srtape, &h->ctape, &h->cwtape, &h->l1tape, &h->kltape})   // checkpoints are states of the solve on the old f: the sweep would recompute on the new one
        if (t->spacing) t->valid = false;
    return BPLTV_OK;
}

int bpltv_set_data(bpltv_t* h, const double* ubar, const double* f) {
    if (h && h->multi) return multi_set_data(h, ubar, f);
    return set_data_impl(h, ubar, f, hipMemcpyHostToDevice);
}

int bpltv_set_data_device(bpltv_t* h, const double* d_ubar, const double* d_f) {
    if (h && h->multi) {
        const int r = multi_forward0(h, "bpltv_set_data_device", [&](bpltv_t* c) { return bpltv_set_data_device(c, d_ubar, d_f); });
        if (r == BPLTV_OK) h->has_data = true;
        return r;
    }
    return set_data_impl(h, d_ubar, d_f, hipMemcpyDeviceToDevice);
}

int bpltv_denoise(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_denoise(h, alpha, am, an, pp, u_out);
    return denoise_common(h, false, alpha, false, am, an, 1, pp, u_out);
}

int bpltv_denoise_device(bpltv_t* h, const double* d_alpha, int am, int an, const bpltv_params* pp) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return multi_forward0_solve(h, "bpltv_denoise_device", [&](bpltv_t* c) { return bpltv_denoise_device(c, d_alpha, am, an, pp); });
    return denoise_common(h, false, d_alpha, true, am, an, 1, pp, nullptr);
}

// bpltv_denoise / bpltv_denoise_device with one parameter block per image: upload_alpha with O blocks, after which the
// PDHG and gap kernels of the dataset context address block k for image k (h->alpha_istride).
int bpltv_denoise_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_denoise(h, alphas, am, an, pp, u_out, 1, true);
    return denoise_common(h, false, alphas, false, am, an, h->O, pp, u_out);
}

int bpltv_denoise_each_device(bpltv_t* h, const double* d_alphas, int am, int an, const bpltv_params* pp) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return multi_forward0_solve(h, "bpltv_denoise_each_device", [&](bpltv_t* c) { return bpltv_denoise_each_device(c, d_alphas, am, an, pp); });
    return denoise_common(h, false, d_alphas, true, am, an, h->O, pp, nullptr);
}

int bpltv_evaluate(bpltv_t* h, const double* alpha, int am, int an, double delta, const bpltv_params* p,
                   double* u_out, double* cost_out, double* grad_out) {
    if (!h) return BPLTV_E_ARG;
    if (!cost_out || !grad_out) return set_err(h, BPLTV_E_ARG, "evaluate: null output pointer");
    if (am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "alpha: empty shape");
    std::vector<double> part(1 + (size_t)am * an);
    int rc = h->multi ? multi_evaluate(h, alpha, am, an, delta, p, u_out, part.data())
                      : evaluate_common(h, false, alpha, am, an, delta, p, u_out, nullptr, part.data());
    if (rc) return rc;
    *cost_out = part[0];
    std::memcpy(grad_out, part.data() + 1, sizeof(double) * (size_t)am * an);
    return BPLTV_OK;
}

int bpltv_sumregs_default_params(bpltv_params* p) {
    const int rc = bpltv_default_params(p);   // same solver block (SumRegsLearningFunction.jl:39-55 == TVLearningFunctionVec.jl:33-43)
    if (rc) return rc;
    p->delta_t = 1e-3;                        // SumRegsLearningFunction.jl:8,22
    return BPLTV_OK;
}

int bpltv_sumregs_denoise(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_denoise(h, alpha, am, an, pp, u_out, 3);
    return denoise_common(h, true, alpha, false, am, an, 1, pp, u_out);
}

int bpltv_sumregs_denoise_device(bpltv_t* h, const double* d_alpha, int am, int an, const bpltv_params* pp) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return multi_forward0_solve(h, "bpltv_sumregs_denoise_device", [&](bpltv_t* c) { return bpltv_sumregs_denoise_device(c, d_alpha, am, an, pp); });
    return denoise_common(h, true, d_alpha, true, am, an, 1, pp, nullptr);
}

// bpltv_sumregs_denoise / bpltv_sumregs_denoise_device with one parameter block (three slices) per image: upload_alpha with
// O blocks, after which the PDHG and gap kernels of the dataset context address block k for image k (h->alpha_istride).
int bpltv_sumregs_denoise_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_denoise(h, alphas, am, an, pp, u_out, 3, true);
    return denoise_common(h, true, alphas, false, am, an, h->O, pp, u_out);
}

int bpltv_sumregs_denoise_each_device(bpltv_t* h, const double* d_alphas, int am, int an, const bpltv_params* pp) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return multi_forward0_solve(h, "bpltv_sumregs_denoise_each_device",
                                    [&](bpltv_t* c) { return bpltv_sumregs_denoise_each_device(c, d_alphas, am, an, pp); });
    return denoise_common(h, true, d_alphas, true, am, an, h->O, pp, nullptr);
}

int bpltv_sumregs_evaluate(bpltv_t* h, const double* alpha, int am, int an, double delta, const bpltv_params* pp, double* u_out,
                           double* cost_out, double* grad_out) {
    if (!h) return BPLTV_E_ARG;
    if (!cost_out || !grad_out) return set_err(h, BPLTV_E_ARG, "evaluate: null output pointer");
    if (!alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "alpha: null pointer or empty shape");
    const bpltv_params p = resolve(pp, true);
    std::vector<double> part(1 + 3 * (size_t)am * an);
    int rc = h->multi ? multi_evaluate(h, alpha, am, an, delta, &p, u_out, part.data(), 3)
                      : evaluate_common(h, true, alpha, am, an, delta, &p, u_out, nullptr, part.data());
    if (rc) return rc;
    *cost_out = part[0];
    std::memcpy(grad_out, part.data() + 1, sizeof(double) * 3 * (size_t)am * an);
    return BPLTV_OK;
}

int bpltv_evaluate_partial(bpltv_t* h, const double* alpha, int am, int an, double delta, const bpltv_params* p,
                           double* u_out, double* partial_out) {
    if (!h) return BPLTV_E_ARG;
    if (!partial_out) return set_err(h, BPLTV_E_ARG, "evaluate_partial: null output pointer");
    if (h->multi) {   // the "partial" of a multi-device handle is the total over its shards
        if (!alpha || am < 1 || an < 1) return set_err(h, BPLTV_E_ARG, "alpha: null pointer or empty shape");
        return multi_evaluate(h, alpha, am, an, delta, p, u_out, partial_out);
    }
    return evaluate_common(h, false, alpha, am, an, delta, p, u_out, nullptr, partial_out);
}

int bpltv_evaluate_device(bpltv_t* h, const double* alpha, int am, int an, double delta, const bpltv_params* p,
                          double* d_partial) {
    if (!h) return BPLTV_E_ARG;
    if (!d_partial) return set_err(h, BPLTV_E_ARG, "evaluate_device: null output pointer");
    if (h->multi)
        return multi_forward0_solve(h, "bpltv_evaluate_device", [&](bpltv_t* c) { return bpltv_evaluate_device(c, alpha, am, an, delta, p, d_partial); });
    return evaluate_common(h, false, alpha, am, an, delta, p, nullptr, d_partial, nullptr);
}

int bpltv_weighted_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                           double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, "bpltv_weighted_denoise", true, [&](bpltv_t* c) { return bpltv_weighted_denoise(c, w, wo, alpha, am, an, pp, u_out); });
    return weighted_denoise_common(h, w, wo, alpha, false, am, an, pp, u_out);
}

int bpltv_weighted_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                  const bpltv_params* pp) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, "bpltv_weighted_denoise_device", true, [&](bpltv_t* c) { return bpltv_weighted_denoise_device(c, d_w, wo, d_alpha, am, an, pp); });
    return weighted_denoise_common(h, d_w, wo, d_alpha, true, am, an, pp, nullptr);
}

int bpltv_weighted_vjp(bpltv_t* h, const double* u, const double* f, const double* w, int wo, const double* alpha, int am, int an,
                       const bpltv_params* pp, const double* gu, double* grad_f_out, double* grad_alpha_out, double* grad_w_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, "bpltv_weighted_vjp", false, [&](bpltv_t* c) {
            return bpltv_weighted_vjp(c, u, f, w, wo, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, grad_w_out);
        });
    if (!u || !gu || !w || !alpha) return set_err(h, BPLTV_E_ARG, "weighted_vjp: null pointer");
    if (!grad_f_out && !grad_alpha_out && !grad_w_out) return set_err(h, BPLTV_E_ARG, "weighted_vjp: all three outputs are NULL");
    if (grad_w_out && !f) return set_err(h, BPLTV_E_ARG, "weighted_vjp: grad_w = -(u - f) o p needs f");
    if (wo != 1 && wo != h->O) return set_err(h, BPLTV_E_ARG, "weighted_vjp: wo = %d: one weight plane (1) or one per image (%d)", wo, h->O);
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "weighted_vjp: parameter shape %dx%d (image %dx%d)", am, an, h->M, h->N);
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t tot = h->tot, P = (size_t)am * an, nw = (size_t)wo * h->npx;
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, tot * sizeof(double)));
    }
    if (grad_f_out && !h->d_gf2) HIPCHK(h, hipMalloc((void**)&h->d_gf2, tot * sizeof(double)));
    if (grad_w_out && !h->d_wst) HIPCHK(h, hipMalloc((void**)&h->d_wst, 2 * tot * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(h->d_u2, u, tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar2, gu, tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (grad_w_out) HIPCHK(h, hipMemcpyAsync(h->d_wst, f, tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = ensure(h, &h->d_vjp, &h->vjp_cap, 4 + 2 * P + nw);
    if (rc) return rc;
    double* d_ga = grad_alpha_out ? h->d_vjp + 4 + P : nullptr;
    double* d_gw = grad_w_out ? h->d_wst + tot : nullptr;
    rc = weighted_vjp_common(h, h->d_u2, grad_w_out ? h->d_wst : nullptr, w, wo, alpha, false, am, an, pp, h->d_ubar2,
                             grad_f_out ? h->d_gf2 : nullptr, d_ga, d_gw);
    if (rc) return rc;
    if (grad_f_out) HIPCHK(h, hipMemcpyAsync(grad_f_out, h->d_gf2, tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_alpha_out) HIPCHK(h, hipMemcpyAsync(grad_alpha_out, d_ga, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_w_out) HIPCHK(h, hipMemcpyAsync(grad_w_out, d_gw, nw * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

int bpltv_weighted_vjp_device(bpltv_t* h, const double* d_u, const double* d_f, const double* d_w, int wo, const double* d_alpha,
                              int am, int an, const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha,
                              double* d_grad_w) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, "bpltv_weighted_vjp_device", false, [&](bpltv_t* c) {
            return bpltv_weighted_vjp_device(c, d_u, d_f, d_w, wo, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha, d_grad_w);
        });
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = weighted_vjp_common(h, d_u, d_f, d_w, wo, d_alpha, true, am, an, pp, d_gu, d_grad_f, d_grad_alpha, d_grad_w);
    if (rc) return rc;
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// The taped solves and their sweeps (TV, weighted, sum of regularisers: TapedModel): one helper per kind behind the entry points
static int tape_doubles_entry(bpltv_t* h, const TapedModel& m, const char* what, const bpltv_params* pp, unsigned long long* n_out) {
    if (!h) return BPLTV_E_ARG;
    if (!n_out) return set_err(h, BPLTV_E_ARG, "%s: null pointer", what);
    const bpltv_params p = resolve(pp, m.slices == 3);
    if (p.maxiter < 1) return set_err(h, BPLTV_E_ARG, "%s: maxiter = %d (at least one iteration)", what, p.maxiter);
    const int C = tape_spacing(m, p.maxiter, h->opt.tape_checkpoint);   // checkpoints: one state set per segment
    const unsigned long long planes = C ? (unsigned long long)m.nplanes * tape_segments(p.maxiter, C) : (unsigned long long)m.tape_planes * p.maxiter;
    *n_out = planes * (unsigned long long)h->M * h->N * h->O;
    return BPLTV_OK;
}

static int taped_denoise_entry(bpltv_t* h, const TapedModel& m, const char* what, const double* w, int wo, const double* alpha, bool dev,
                               int am, int an, const bpltv_params* pp, double* d_tape, double* u_out, bool each) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, true, [&](bpltv_t* c) { return taped_denoise_entry(c, m, what, w, wo, alpha, dev, am, an, pp, d_tape, u_out, each); },
                              m.multi_name);
    return taped_denoise(h, m, w, wo, alpha, dev, am, an, pp, d_tape, u_out, each);
}

// The host forms of the sweeps on a single-device handle: the host arrays staged around taped_vjp, on the handle's tape
static int taped_vjp_host(bpltv_t* h, const TapedModel& m, const double* w, int wo, const double* alpha, int am, int an,
                          const bpltv_params* pp, const double* gu, double* grad_f_out, double* grad_alpha_out, double* grad_w_out, bool each) {
    const char* who = m.slices == 3 ? "unrolled_vjp" : m.vjp;   // (what the messages of these checks have always said)
    if (!gu || !alpha || (m.weighted && !w)) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (!grad_f_out && !grad_alpha_out && !grad_w_out)
        return set_err(h, BPLTV_E_ARG, "%s: %s outputs are NULL", who, m.weighted ? "all three" : "both");
    if (m.weighted && wo != 1 && wo != h->O)
        return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, wo, h->O);
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "%s: parameter shape %dx%d (image %dx%d)", who, am, an, h->M, h->N);
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t tot = h->tot, P = (size_t)m.slices * am * an * (each ? h->O : 1), nw = m.weighted ? (size_t)wo * h->npx : 0;
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, tot * sizeof(double)));
    }
    if (grad_f_out && !h->d_gf2) HIPCHK(h, hipMalloc((void**)&h->d_gf2, tot * sizeof(double)));
    if (grad_w_out && !h->d_wst) HIPCHK(h, hipMalloc((void**)&h->d_wst, 2 * tot * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar2, gu, tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = ensure(h, &h->d_vjp, &h->vjp_cap, 4 + 2 * P + nw);
    if (rc) return rc;
    double* d_ga = grad_alpha_out ? h->d_vjp + 4 + P : nullptr;
    double* d_gw = grad_w_out ? h->d_wst + tot : nullptr;
    rc = taped_vjp(h, m, nullptr, w, wo, alpha, false, am, an, pp, h->d_ubar2, grad_f_out ? h->d_gf2 : nullptr, d_ga, d_gw, each);
    if (rc) return rc;
    if (grad_f_out) HIPCHK(h, hipMemcpyAsync(grad_f_out, h->d_gf2, tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_alpha_out) HIPCHK(h, hipMemcpyAsync(grad_alpha_out, d_ga, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_w_out) HIPCHK(h, hipMemcpyAsync(grad_w_out, d_gw, nw * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (m.tv_stats) h->st.total_ms = wt.ms();   // (the other two models' sweeps change adjoint_ms and adjoint_method only)
    return BPLTV_OK;
}

static int taped_vjp_entry(bpltv_t* h, const TapedModel& m, const char* what, bool dev, const double* d_tape, const double* w, int wo,
                           const double* alpha, int am, int an, const bpltv_params* pp, const double* gu, double* grad_f, double* grad_alpha,
                           double* grad_w, bool each) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, false, [&](bpltv_t* c) {
            return taped_vjp_entry(c, m, what, dev, d_tape, w, wo, alpha, am, an, pp, gu, grad_f, grad_alpha, grad_w, each);
        }, m.multi_name);
    if (!dev) return taped_vjp_host(h, m, w, wo, alpha, am, an, pp, gu, grad_f, grad_alpha, grad_w, each);
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = taped_vjp(h, m, d_tape, w, wo, alpha, true, am, an, pp, gu, grad_f, grad_alpha, grad_w, each);
    if (rc) return rc;
    if (m.tv_stats) h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

int bpltv_unrolled_tape_doubles(bpltv_t* h, const bpltv_params* pp, unsigned long long* n_out) {
    return tape_doubles_entry(h, kTapedTV, "bpltv_unrolled_tape_doubles", pp, n_out);
}
int bpltv_unrolled_denoise(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedTV, "bpltv_unrolled_denoise", nullptr, 1, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_unrolled_denoise_device(bpltv_t* h, const double* d_alpha, int am, int an, const bpltv_params* pp, double* d_tape) {
    return taped_denoise_entry(h, kTapedTV, "bpltv_unrolled_denoise_device", nullptr, 1, d_alpha, true, am, an, pp, d_tape, nullptr, false);
}
// bpltv_unrolled_denoise with one parameter block per image: upload_alpha with O blocks, after which the taped kernel and the
// gap kernels address block k for image k (h->alpha_istride); the tape remembers it (Tape::each).
int bpltv_unrolled_denoise_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedTV, "bpltv_unrolled_denoise_each", nullptr, 1, alphas, false, am, an, pp, nullptr, u_out, true);
}
int bpltv_unrolled_denoise_each_device(bpltv_t* h, const double* d_alphas, int am, int an, const bpltv_params* pp, double* d_tape) {
    return taped_denoise_entry(h, kTapedTV, "bpltv_unrolled_denoise_each_device", nullptr, 1, d_alphas, true, am, an, pp, d_tape, nullptr, true);
}
int bpltv_unrolled_vjp(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, const double* gu,
                       double* grad_f_out, double* grad_alpha_out) {
    return taped_vjp_entry(h, kTapedTV, "bpltv_unrolled_vjp", false, nullptr, nullptr, 1, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, nullptr, false);
}
int bpltv_unrolled_vjp_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, const double* gu,
                            double* grad_f_out, double* grad_alphas_out) {
    return taped_vjp_entry(h, kTapedTV, "bpltv_unrolled_vjp_each", false, nullptr, nullptr, 1, alphas, am, an, pp, gu, grad_f_out, grad_alphas_out, nullptr, true);
}
int bpltv_unrolled_vjp_each_device(bpltv_t* h, const double* d_tape, const double* d_alphas, int am, int an, const bpltv_params* pp,
                                   const double* d_gu, double* d_grad_f, double* d_grad_alphas) {
    return taped_vjp_entry(h, kTapedTV, "bpltv_unrolled_vjp_each_device", true, d_tape, nullptr, 1, d_alphas, am, an, pp, d_gu, d_grad_f, d_grad_alphas, nullptr, true);
}
int bpltv_unrolled_vjp_device(bpltv_t* h, const double* d_tape, const double* d_alpha, int am, int an, const bpltv_params* pp,
                              const double* d_gu, double* d_grad_f, double* d_grad_alpha) {
    return taped_vjp_entry(h, kTapedTV, "bpltv_unrolled_vjp_device", true, d_tape, nullptr, 1, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha, nullptr, false);
}

int bpltv_sumregs_unrolled_tape_doubles(bpltv_t* h, const bpltv_params* pp, unsigned long long* n_out) {
    return tape_doubles_entry(h, kTapedSr, "bpltv_sumregs_unrolled_tape_doubles", pp, n_out);
}
int bpltv_sumregs_unrolled_denoise(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedSr, "bpltv_sumregs_unrolled_denoise", nullptr, 1, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_sumregs_unrolled_denoise_device(bpltv_t* h, const double* d_alpha, int am, int an, const bpltv_params* pp, double* d_tape) {
    return taped_denoise_entry(h, kTapedSr, "bpltv_sumregs_unrolled_denoise_device", nullptr, 1, d_alpha, true, am, an, pp, d_tape, nullptr, false);
}
int bpltv_sumregs_unrolled_denoise_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedSr, "bpltv_sumregs_unrolled_denoise_each", nullptr, 1, alphas, false, am, an, pp, nullptr, u_out, true);
}
int bpltv_sumregs_unrolled_denoise_each_device(bpltv_t* h, const double* d_alphas, int am, int an, const bpltv_params* pp, double* d_tape) {
    return taped_denoise_entry(h, kTapedSr, "bpltv_sumregs_unrolled_denoise_each_device", nullptr, 1, d_alphas, true, am, an, pp, d_tape, nullptr, true);
}
int bpltv_sumregs_unrolled_vjp(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, const double* gu,
                               double* grad_f_out, double* grad_alpha_out) {
    return taped_vjp_entry(h, kTapedSr, "bpltv_sumregs_unrolled_vjp", false, nullptr, nullptr, 1, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, nullptr, false);
}
int bpltv_sumregs_unrolled_vjp_device(bpltv_t* h, const double* d_tape, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                      const double* d_gu, double* d_grad_f, double* d_grad_alpha) {
    return taped_vjp_entry(h, kTapedSr, "bpltv_sumregs_unrolled_vjp_device", true, d_tape, nullptr, 1, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha, nullptr, false);
}
int bpltv_sumregs_unrolled_vjp_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, const double* gu,
                                    double* grad_f_out, double* grad_alphas_out) {
    return taped_vjp_entry(h, kTapedSr, "bpltv_sumregs_unrolled_vjp_each", false, nullptr, nullptr, 1, alphas, am, an, pp, gu, grad_f_out, grad_alphas_out, nullptr, true);
}
int bpltv_sumregs_unrolled_vjp_each_device(bpltv_t* h, const double* d_tape, const double* d_alphas, int am, int an, const bpltv_params* pp,
                                           const double* d_gu, double* d_grad_f, double* d_grad_alphas) {
    return taped_vjp_entry(h, kTapedSr, "bpltv_sumregs_unrolled_vjp_each_device", true, d_tape, nullptr, 1, d_alphas, am, an, pp, d_gu, d_grad_f, d_grad_alphas, nullptr, true);
}

// The channel-coupled model: channels picks the instance; a colour image is `channels` consecutive planes
static const TapedModel* color_model(bpltv_t* h, const char* what, int channels, int* rc, bool weighted = false) {
    *rc = BPLTV_OK;
    if (channels < 1 || channels > COLOR_MAX_C) {
        *rc = set_err(h, BPLTV_E_ARG, "%s: channels = %d (1 ... %d)", what, channels, COLOR_MAX_C);
        return nullptr;
    }
    if (!h->multi && h->O % channels != 0) {   // (a forwarding handle leaves it to its shard)
        *rc = set_err(h, BPLTV_E_ARG, "%s: channels = %d does not divide the handle's %d planes", what, channels, h->O);
        return nullptr;
    }
    return weighted ? &kTapedColorWeighted[channels - 1] : &kTapedColor[channels - 1];
}
// w != nullptr or weighted: the weighted form (a null w is its own rejection, after the channels')
static int color_denoise_entry(bpltv_t* h, const char* what, int channels, const double* alpha, bool dev, int am, int an, const bpltv_params* pp,
                               double* d_tape, double* u_out, bool taped, bool weighted = false, const double* w = nullptr, int wo = 1) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    const TapedModel* m = color_model(h, what, channels, &rc, weighted);
    if (!m) return rc;
    if (h->multi)
        return weighted_multi(h, what, true, [&](bpltv_t* c) {
            return color_denoise_entry(c, what, channels, alpha, dev, am, an, pp, d_tape, u_out, taped, weighted, w, wo);
        }, m->multi_name);
    return taped_denoise(h, *m, w, wo, alpha, dev, am, an, pp, d_tape, u_out, false, taped);
}
int bpltv_color_denoise(bpltv_t* h, int channels, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return color_denoise_entry(h, "bpltv_color_denoise", channels, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_color_denoise_device(bpltv_t* h, int channels, const double* d_alpha, int am, int an, const bpltv_params* pp) {
    return color_denoise_entry(h, "bpltv_color_denoise_device", channels, d_alpha, true, am, an, pp, nullptr, nullptr, false);
}
int bpltv_color_unrolled_denoise(bpltv_t* h, int channels, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return color_denoise_entry(h, "bpltv_color_unrolled_denoise", channels, alpha, false, am, an, pp, nullptr, u_out, true);
}
int bpltv_color_unrolled_denoise_device(bpltv_t* h, int channels, const double* d_alpha, int am, int an, const bpltv_params* pp, double* d_tape) {
    return color_denoise_entry(h, "bpltv_color_unrolled_denoise_device", channels, d_alpha, true, am, an, pp, d_tape, nullptr, true);
}
int bpltv_color_unrolled_vjp(bpltv_t* h, int channels, const double* alpha, int am, int an, const bpltv_params* pp, const double* gu, double* grad_f_out,
                             double* grad_alpha_out) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    const TapedModel* m = color_model(h, "bpltv_color_unrolled_vjp", channels, &rc);
    if (!m) return rc;
    return taped_vjp_entry(h, *m, "bpltv_color_unrolled_vjp", false, nullptr, nullptr, 1, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, nullptr, false);
}
int bpltv_color_unrolled_vjp_device(bpltv_t* h, int channels, const double* d_tape, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                    const double* d_gu, double* d_grad_f, double* d_grad_alpha) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    const TapedModel* m = color_model(h, "bpltv_color_unrolled_vjp_device", channels, &rc);
    if (!m) return rc;
    return taped_vjp_entry(h, *m, "bpltv_color_unrolled_vjp_device", true, d_tape, nullptr, 1, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha, nullptr, false);
}

// The weighted channel-coupled model
int bpltv_color_weighted_denoise(bpltv_t* h, int channels, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                 double* u_out) {
    return color_denoise_entry(h, "bpltv_color_weighted_denoise", channels, alpha, false, am, an, pp, nullptr, u_out, false, true, w, wo);
}
int bpltv_color_weighted_denoise_device(bpltv_t* h, int channels, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                        const bpltv_params* pp) {
    return color_denoise_entry(h, "bpltv_color_weighted_denoise_device", channels, d_alpha, true, am, an, pp, nullptr, nullptr, false, true, d_w, wo);
}
int bpltv_color_weighted_unrolled_denoise(bpltv_t* h, int channels, const double* w, int wo, const double* alpha, int am, int an,
                                          const bpltv_params* pp, double* u_out) {
    return color_denoise_entry(h, "bpltv_color_weighted_unrolled_denoise", channels, alpha, false, am, an, pp, nullptr, u_out, true, true, w, wo);
}
int bpltv_color_weighted_unrolled_denoise_device(bpltv_t* h, int channels, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                                 const bpltv_params* pp, double* d_tape) {
    return color_denoise_entry(h, "bpltv_color_weighted_unrolled_denoise_device", channels, d_alpha, true, am, an, pp, d_tape, nullptr, true, true, d_w,
                               wo);
}
int bpltv_color_weighted_unrolled_vjp(bpltv_t* h, int channels, const double* w, int wo, const double* alpha, int am, int an,
                                      const bpltv_params* pp, const double* gu, double* grad_f_out, double* grad_alpha_out, double* grad_w_out) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    const TapedModel* m = color_model(h, "bpltv_color_weighted_unrolled_vjp", channels, &rc, true);
    if (!m) return rc;
    return taped_vjp_entry(h, *m, "bpltv_color_weighted_unrolled_vjp", false, nullptr, w, wo, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out,
                           grad_w_out, false);
}
int bpltv_color_weighted_unrolled_vjp_device(bpltv_t* h, int channels, const double* d_tape, const double* d_w, int wo, const double* d_alpha,
                                             int am, int an, const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha,
                                             double* d_grad_w) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    const TapedModel* m = color_model(h, "bpltv_color_weighted_unrolled_vjp_device", channels, &rc, true);
    if (!m) return rc;
    return taped_vjp_entry(h, *m, "bpltv_color_weighted_unrolled_vjp_device", true, d_tape, d_w, wo, d_alpha, am, an, pp, d_gu, d_grad_f,
                           d_grad_alpha, d_grad_w, false);
}

int bpltv_weighted_unrolled_tape_doubles(bpltv_t* h, const bpltv_params* pp, unsigned long long* n_out) {
    return tape_doubles_entry(h, kTapedWeighted, "bpltv_weighted_unrolled_tape_doubles", pp, n_out);
}
int bpltv_weighted_unrolled_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                    double* u_out) {
    return taped_denoise_entry(h, kTapedWeighted, "bpltv_weighted_unrolled_denoise", w, wo, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_weighted_unrolled_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                           const bpltv_params* pp, double* d_tape) {
    return taped_denoise_entry(h, kTapedWeighted, "bpltv_weighted_unrolled_denoise_device", d_w, wo, d_alpha, true, am, an, pp, d_tape, nullptr, false);
}
int bpltv_weighted_unrolled_vjp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                const double* gu, double* grad_f_out, double* grad_alpha_out, double* grad_w_out) {
    return taped_vjp_entry(h, kTapedWeighted, "bpltv_weighted_unrolled_vjp", false, nullptr, w, wo, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out,
                           grad_w_out, false);
}
int bpltv_weighted_unrolled_vjp_device(bpltv_t* h, const double* d_tape, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                       const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha,
                                       double* d_grad_w) {
    return taped_vjp_entry(h, kTapedWeighted, "bpltv_weighted_unrolled_vjp_device", true, d_tape, d_w, wo, d_alpha, am, an, pp, d_gu, d_grad_f,
                           d_grad_alpha, d_grad_w, false);
}

// The TV-L1 model: the plain solve is the taped solve's launches of the no-tape instantiation
static int l1_denoise_entry(bpltv_t* h, const char* what, const double* w, int wo, const double* alpha, bool dev, int am, int an,
                            const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, true, [&](bpltv_t* c) { return l1_denoise_entry(c, what, w, wo, alpha, dev, am, an, pp, u_out); },
                              kTapedL1.multi_name);
    return taped_denoise(h, kTapedL1, w, wo, alpha, dev, am, an, pp, nullptr, u_out, false, false);
}
int bpltv_lone_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return l1_denoise_entry(h, "bpltv_lone_denoise", w, wo, alpha, false, am, an, pp, u_out);
}
int bpltv_lone_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp) {
    return l1_denoise_entry(h, "bpltv_lone_denoise_device", d_w, wo, d_alpha, true, am, an, pp, nullptr);
}
int bpltv_lone_unrolled_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedL1, "bpltv_lone_unrolled_denoise", w, wo, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_lone_unrolled_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                     double* d_tape) {
    return taped_denoise_entry(h, kTapedL1, "bpltv_lone_unrolled_denoise_device", d_w, wo, d_alpha, true, am, an, pp, d_tape, nullptr, false);
}
int bpltv_lone_unrolled_vjp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, const double* gu,
                          double* grad_f_out, double* grad_alpha_out, double* grad_w_out) {
    return taped_vjp_entry(h, kTapedL1, "bpltv_lone_unrolled_vjp", false, nullptr, w, wo, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, grad_w_out,
                           false);
}
int bpltv_lone_unrolled_vjp_device(bpltv_t* h, const double* d_tape, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                 const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha, double* d_grad_w) {
    return taped_vjp_entry(h, kTapedL1, "bpltv_lone_unrolled_vjp_device", true, d_tape, d_w, wo, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha,
                           d_grad_w, false);
}

// The TV-KL model, as the TV-L1 model's entry points
static int kl_denoise_entry(bpltv_t* h, const char* what, const double* w, int wo, const double* alpha, bool dev, int am, int an,
                            const bpltv_params* pp, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, true, [&](bpltv_t* c) { return kl_denoise_entry(c, what, w, wo, alpha, dev, am, an, pp, u_out); },
                              kTapedKL.multi_name);
    return taped_denoise(h, kTapedKL, w, wo, alpha, dev, am, an, pp, nullptr, u_out, false, false);
}
int bpltv_kl_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return kl_denoise_entry(h, "bpltv_kl_denoise", w, wo, alpha, false, am, an, pp, u_out);
}
int bpltv_kl_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp) {
    return kl_denoise_entry(h, "bpltv_kl_denoise_device", d_w, wo, d_alpha, true, am, an, pp, nullptr);
}
int bpltv_kl_unrolled_denoise(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, double* u_out) {
    return taped_denoise_entry(h, kTapedKL, "bpltv_kl_unrolled_denoise", w, wo, alpha, false, am, an, pp, nullptr, u_out, false);
}
int bpltv_kl_unrolled_denoise_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                     double* d_tape) {
    return taped_denoise_entry(h, kTapedKL, "bpltv_kl_unrolled_denoise_device", d_w, wo, d_alpha, true, am, an, pp, d_tape, nullptr, false);
}
int bpltv_kl_unrolled_vjp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, const double* gu,
                          double* grad_f_out, double* grad_alpha_out, double* grad_w_out) {
    return taped_vjp_entry(h, kTapedKL, "bpltv_kl_unrolled_vjp", false, nullptr, w, wo, alpha, am, an, pp, gu, grad_f_out, grad_alpha_out, grad_w_out,
                           false);
}
int bpltv_kl_unrolled_vjp_device(bpltv_t* h, const double* d_tape, const double* d_w, int wo, const double* d_alpha, int am, int an,
                                 const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha, double* d_grad_w) {
    return taped_vjp_entry(h, kTapedKL, "bpltv_kl_unrolled_vjp_device", true, d_tape, d_w, wo, d_alpha, am, an, pp, d_gu, d_grad_f, d_grad_alpha,
                           d_grad_w, false);
}

// bpltv_unrolled_jvp, bpltv_unrolled_jvp_each and bpltv_weighted_unrolled_jvp on a single-device handle: the host arrays
// staged around unrolled_jvp_common.  W (nullable: the TV model): the weighted model's host w and host dw.
static int unrolled_jvp_host(bpltv_t* h, const char* who, const double* alpha, int am, int an, const bpltv_params* pp, int ndir, const double* df,
                             const double* dalpha, double* du_out, double* u_out, bool each, const JvpWeight* W, int channels = 0) {
    const double* dw = W ? W->dw : nullptr;
    if (!alpha || !du_out || (W && !W->w)) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (ndir < 1) return set_err(h, BPLTV_E_ARG, "%s: ndir = %d (at least one direction)", who, ndir);
    if (!df && !dalpha && !dw) return set_err(h, BPLTV_E_ARG, "%s: %s tangents are NULL", who, W ? "all three" : "both");
    if (W && W->wo != 1 && W->wo != h->O)
        return set_err(h, BPLTV_E_ARG, "%s: wo = %d: one weight plane (1) or one per image (%d)", who, W->wo, h->O);
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "%s: parameter shape %dx%d (image %dx%d)", who, am, an, h->M, h->N);
    const size_t nt = (size_t)ndir * h->tot, na = (size_t)ndir * am * an * (each ? h->O : 1), nd = W ? (size_t)ndir * W->wo * h->npx : 0;
    if (int crc = check_tangent_host(h, who, "tangent df", df, nt)) return crc;
    if (int crc = check_tangent_host(h, who, "tangent dalpha", dalpha, na)) return crc;
    if (int crc = check_tangent_host(h, who, "tangent dw", dw, nd)) return crc;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, &h->d_jvp, &h->jvp_cap, 2 * nt + na + h->tot + nd);   // [du | df | dalpha | u | dw]
    if (rc) return rc;
    double *d_du = h->d_jvp, *d_df = df ? h->d_jvp + nt : nullptr, *d_da = dalpha ? h->d_jvp + 2 * nt : nullptr;
    double* d_u = u_out ? h->d_jvp + 2 * nt + na : nullptr;
    double* d_dw = dw ? h->d_jvp + 2 * nt + na + h->tot : nullptr;
    if (df) HIPCHK(h, hipMemcpyAsync(d_df, df, nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (dalpha) HIPCHK(h, hipMemcpyAsync(d_da, dalpha, na * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (dw) HIPCHK(h, hipMemcpyAsync(d_dw, dw, nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    JvpWeight Wd{};
    if (W) Wd = JvpWeight{W->w, W->wo, d_dw, W->data};
    rc = unrolled_jvp_common(h, who, alpha, false, am, an, pp, ndir, d_df, d_da, d_du, d_u, nullptr, each, W ? &Wd : nullptr, channels);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(du_out, d_du, nt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (u_out) HIPCHK(h, hipMemcpyAsync(u_out, d_u, h->tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BPLTV_OK;
}

// the taped model a weighted tangent sweep belongs to (its name on a multi-device handle)
static const TapedModel& jvp_weighted_model(int data) { return data == JVP_L1 ? kTapedL1 : (data == JVP_KL ? kTapedKL : kTapedWeighted); }

static int unrolled_jvp_entry(bpltv_t* h, const char* what, bool dev, const double* alpha, int am, int an, const bpltv_params* pp, int ndir,
                              const double* df, const double* dalpha, double* du, double* u, bool each, const JvpWeight* W = nullptr,
                              int channels = 0) {
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, false, [&](bpltv_t* c) { return unrolled_jvp_entry(c, what, dev, alpha, am, an, pp, ndir, df, dalpha, du, u, each, W, channels); },
                              channels ? kTapedColor[0].multi_name : (W ? jvp_weighted_model(W->data).multi_name : kUnrolled));
    int crc = BPLTV_OK;   // (color_model leaves the division to a forwarding handle's shard: this is where it arrives)
    if (channels && !color_model(h, what, channels, &crc)) return crc;
    const char* who = channels ? "color_unrolled_jvp"
                      : W      ? (W->data == JVP_L1 ? "l1_unrolled_jvp" : W->data == JVP_KL ? "kl_unrolled_jvp" : "weighted_unrolled_jvp")
                               : (each ? "unrolled_jvp_each" : "unrolled_jvp");
    if (!dev) return unrolled_jvp_host(h, who, alpha, am, an, pp, ndir, df, dalpha, du, u, each, W, channels);
    HIPCHK(h, hipSetDevice(h->device));
    return unrolled_jvp_common(h, who, alpha, true, am, an, pp, ndir, df, dalpha, du, u, nullptr, each, W, channels);
}

int bpltv_unrolled_jvp(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, int ndir, const double* df,
                       const double* dalpha, double* du_out, double* u_out) {
    return unrolled_jvp_entry(h, "bpltv_unrolled_jvp", false, alpha, am, an, pp, ndir, df, dalpha, du_out, u_out, false);
}
int bpltv_unrolled_jvp_each(bpltv_t* h, const double* alphas, int am, int an, const bpltv_params* pp, int ndir, const double* df,
                            const double* dalphas, double* du_out, double* u_out) {
    return unrolled_jvp_entry(h, "bpltv_unrolled_jvp_each", false, alphas, am, an, pp, ndir, df, dalphas, du_out, u_out, true);
}
int bpltv_unrolled_jvp_each_device(bpltv_t* h, const double* d_alphas, int am, int an, const bpltv_params* pp, int ndir, const double* d_df,
                                   const double* d_dalphas, double* d_du, double* d_u) {
    return unrolled_jvp_entry(h, "bpltv_unrolled_jvp_each_device", true, d_alphas, am, an, pp, ndir, d_df, d_dalphas, d_du, d_u, true);
}
int bpltv_unrolled_jvp_device(bpltv_t* h, const double* d_alpha, int am, int an, const bpltv_params* pp, int ndir, const double* d_df,
                              const double* d_dalpha, double* d_du, double* d_u) {
    return unrolled_jvp_entry(h, "bpltv_unrolled_jvp_device", true, d_alpha, am, an, pp, ndir, d_df, d_dalpha, d_du, d_u, false);
}
int bpltv_weighted_unrolled_jvp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, int ndir,
                                const double* df, const double* dalpha, const double* dw, double* du_out, double* u_out) {
    const JvpWeight W{w, wo, dw};
    return unrolled_jvp_entry(h, "bpltv_weighted_unrolled_jvp", false, alpha, am, an, pp, ndir, df, dalpha, du_out, u_out, false, &W);
}
int bpltv_weighted_unrolled_jvp_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                       int ndir, const double* d_df, const double* d_dalpha, const double* d_dw, double* d_du, double* d_u) {
    const JvpWeight W{d_w, wo, d_dw};
    return unrolled_jvp_entry(h, "bpltv_weighted_unrolled_jvp_device", true, d_alpha, am, an, pp, ndir, d_df, d_dalpha, d_du, d_u, false, &W);
}

// Gradient and Gauss-Newton Hessian of the K-step loss 0.5||u_K(alpha) - ubar||^2 from P = am*an <= GN_MAXP unit-direction
// tangent sweeps: [J | u_K - ubar] into gn_gram_kernel / gn_final_kernel, as gauss_newton does for the implicit Jacobian.
// w (nullable: the TV model; wo planes on the host): the weighted iterations' loss.
// channels: 0 = the TV and weighted entry points; 1 ... 4 = the channel-coupled model's (the loss runs over all planes).
static int unrolled_gauss_newton_entry(bpltv_t* h, const char* what, const double* w, int wo, const double* alpha, int am, int an,
                                       const bpltv_params* pp, double* cost_out, double* grad_out, double* hess_out, int channels = 0,
                                       int data = JVP_QUADRATIC) {
    const char* who = what + 6;   // (without "bpltv_")
    if (!h) return BPLTV_E_ARG;
    if (h->multi)
        return weighted_multi(h, what, false, [&](bpltv_t* c) {
            return unrolled_gauss_newton_entry(c, what, w, wo, alpha, am, an, pp, cost_out, grad_out, hess_out, channels, data);
        }, channels ? kTapedColor[0].multi_name : (w ? jvp_weighted_model(data).multi_name : kUnrolled));
    int crc = BPLTV_OK;   // (color_model leaves the division to a forwarding handle's shard: this is where it arrives)
    if (channels && !color_model(h, what, channels, &crc)) return crc;
    if (!alpha || !cost_out || !grad_out || !hess_out) return set_err(h, BPLTV_E_ARG, "%s: null pointer", who);
    if (am < 1 || an < 1 || am > h->M || an > h->N)
        return set_err(h, BPLTV_E_ARG, "%s: parameter shape %dx%d (image %dx%d)", who, am, an, h->M, h->N);
    const bool amap = am == h->M && an == h->N && !(h->M == 1 && h->N == 1);
    if (amap || (long)am * an > GN_MAXP)
        return set_err(h, BPLTV_E_UNSUPPORTED, "%s: a scalar or a patch parameter of at most %d entries (got %dx%d%s); use bpltv_%sunrolled_jvp for Jacobian columns",
                       who, GN_MAXP, am, an, amap ? ", a pixel map" : "",
                       channels ? "color_" : (data == JVP_L1 ? "lone_" : data == JVP_KL ? "kl_" : (w ? "weighted_" : "")));
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "%s: bpltv_set_data has not been called", who);
    const int P = am * an;
    const size_t nout = (size_t)P + (size_t)P * P;
    HIPCHK(h, hipSetDevice(h->device));
    // workspace [J: P planes | unit directions P x P | per-image partials P (P + 1) O | grad, H | cost]
    const size_t nJ = (size_t)P * h->tot, npart = (size_t)P * (P + 1) * h->O;
    const size_t need = nJ + (size_t)P * P + npart + nout + 1;
    if (h->jvp_cap < need) {
        if (h->d_jvp) (void)hipFree(h->d_jvp);
        h->d_jvp = nullptr; h->jvp_cap = 0;
        const int arc = alloc_all(h, {{(void**)&h->d_jvp, need * sizeof(double)}}, "unrolled_gauss_newton: workspace of the Jacobian columns");
        if (arc) return arc;
        h->jvp_cap = need;
    }
    double *d_J = h->d_jvp, *d_e = d_J + nJ, *d_part = d_e + (size_t)P * P, *d_out = d_part + npart;
    std::vector<double> eye((size_t)P * P, 0.0);
    for (int j = 0; j < P; ++j) eye[(size_t)j * P + j] = 1.0;
    HIPCHK(h, hipMemcpyAsync(d_e, eye.data(), eye.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (eye is a local)
    const double* d_x = nullptr;
    const JvpWeight W{w, wo, nullptr, data};
    int rc = unrolled_jvp_common(h, who, alpha, false, am, an, pp, P, nullptr, d_e, d_J, nullptr, &d_x, false, w ? &W : nullptr, channels);
    if (rc) return rc;
    h->has_per_image = false;   // compute_cost writes d_perimg and d_red
    rc = compute_cost(h, d_x, h->d_ubar, d_out + nout);
    if (rc) return rc;
    hipLaunchKernelGGL(gn_gram_kernel, dim3(P + 1, P, h->O), dim3(256), 0, h->stream, d_J, d_x, h->d_ubar, (int)h->npx, h->O, P, d_part);
    hipLaunchKernelGGL(gn_final_kernel, dim3((P * (P + 1) + 63) / 64), dim3(64), 0, h->stream, d_part, h->O, P, d_out);
    HIPCHK(h, hipGetLastError());
    std::vector<double> out(nout + 1);
    HIPCHK(h, hipMemcpyAsync(out.data(), d_out, (nout + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(grad_out, out.data(), P * sizeof(double));
    std::memcpy(hess_out, out.data() + P, (size_t)P * P * sizeof(double));
    *cost_out = out[nout];
    return BPLTV_OK;
}
int bpltv_unrolled_gauss_newton(bpltv_t* h, const double* alpha, int am, int an, const bpltv_params* pp, double* cost_out,
                                double* grad_out, double* hess_out) {
    return unrolled_gauss_newton_entry(h, "bpltv_unrolled_gauss_newton", nullptr, 1, alpha, am, an, pp, cost_out, grad_out, hess_out);
}
int bpltv_weighted_unrolled_gauss_newton(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                         double* cost_out, double* grad_out, double* hess_out) {
    if (!h) return BPLTV_E_ARG;
    if (!w) return set_err(h, BPLTV_E_ARG, "weighted_unrolled_gauss_newton: w is a null pointer");
    return unrolled_gauss_newton_entry(h, "bpltv_weighted_unrolled_gauss_newton", w, wo, alpha, am, an, pp, cost_out, grad_out, hess_out);
}

// Forward mode through the TV-L1 and the TV-KL iterations (tv_tile_kernel<1,0,1,L1> and <1,0,1,0,KL>):
// the weighted sweep's driver, workspace and contract with the model's data term, step table (gamma = 0) and graphs
int bpltv_lone_unrolled_jvp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, int ndir,
                            const double* df, const double* dalpha, const double* dw, double* du_out, double* u_out) {
    const JvpWeight W{w, wo, dw, JVP_L1};
    return unrolled_jvp_entry(h, "bpltv_lone_unrolled_jvp", false, alpha, am, an, pp, ndir, df, dalpha, du_out, u_out, false, &W);
}
int bpltv_lone_unrolled_jvp_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                   int ndir, const double* d_df, const double* d_dalpha, const double* d_dw, double* d_du, double* d_u) {
    const JvpWeight W{d_w, wo, d_dw, JVP_L1};
    return unrolled_jvp_entry(h, "bpltv_lone_unrolled_jvp_device", true, d_alpha, am, an, pp, ndir, d_df, d_dalpha, d_du, d_u, false, &W);
}
int bpltv_lone_unrolled_gauss_newton(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                     double* cost_out, double* grad_out, double* hess_out) {
    if (!h) return BPLTV_E_ARG;
    if (!w) return set_err(h, BPLTV_E_ARG, "lone_unrolled_gauss_newton: w is a null pointer");
    return unrolled_gauss_newton_entry(h, "bpltv_lone_unrolled_gauss_newton", w, wo, alpha, am, an, pp, cost_out, grad_out, hess_out, 0, JVP_L1);
}
int bpltv_kl_unrolled_jvp(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp, int ndir,
                          const double* df, const double* dalpha, const double* dw, double* du_out, double* u_out) {
    const JvpWeight W{w, wo, dw, JVP_KL};
    return unrolled_jvp_entry(h, "bpltv_kl_unrolled_jvp", false, alpha, am, an, pp, ndir, df, dalpha, du_out, u_out, false, &W);
}
int bpltv_kl_unrolled_jvp_device(bpltv_t* h, const double* d_w, int wo, const double* d_alpha, int am, int an, const bpltv_params* pp,
                                 int ndir, const double* d_df, const double* d_dalpha, const double* d_dw, double* d_du, double* d_u) {
    const JvpWeight W{d_w, wo, d_dw, JVP_KL};
    return unrolled_jvp_entry(h, "bpltv_kl_unrolled_jvp_device", true, d_alpha, am, an, pp, ndir, d_df, d_dalpha, d_du, d_u, false, &W);
}
int bpltv_kl_unrolled_gauss_newton(bpltv_t* h, const double* w, int wo, const double* alpha, int am, int an, const bpltv_params* pp,
                                   double* cost_out, double* grad_out, double* hess_out) {
    if (!h) return BPLTV_E_ARG;
    if (!w) return set_err(h, BPLTV_E_ARG, "kl_unrolled_gauss_newton: w is a null pointer");
    return unrolled_gauss_newton_entry(h, "bpltv_kl_unrolled_gauss_newton", w, wo, alpha, am, an, pp, cost_out, grad_out, hess_out, 0, JVP_KL);
}

// Forward mode through the channel-coupled iterations (color_tangent_tile_kernel)
int bpltv_color_unrolled_jvp(bpltv_t* h, int channels, const double* alpha, int am, int an, const bpltv_params* pp, int ndir, const double* df,
                             const double* dalpha, double* du_out, double* u_out) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    if (!color_model(h, "bpltv_color_unrolled_jvp", channels, &rc)) return rc;
    return unrolled_jvp_entry(h, "bpltv_color_unrolled_jvp", false, alpha, am, an, pp, ndir, df, dalpha, du_out, u_out, false, nullptr, channels);
}
int bpltv_color_unrolled_jvp_device(bpltv_t* h, int channels, const double* d_alpha, int am, int an, const bpltv_params* pp, int ndir,
                                    const double* d_df, const double* d_dalpha, double* d_du, double* d_u) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    if (!color_model(h, "bpltv_color_unrolled_jvp_device", channels, &rc)) return rc;
    return unrolled_jvp_entry(h, "bpltv_color_unrolled_jvp_device", true, d_alpha, am, an, pp, ndir, d_df, d_dalpha, d_du, d_u, false, nullptr, channels);
}
int bpltv_color_unrolled_gauss_newton(bpltv_t* h, int channels, const double* alpha, int am, int an, const bpltv_params* pp, double* cost_out,
                                      double* grad_out, double* hess_out) {
    if (!h) return BPLTV_E_ARG;
    int rc = BPLTV_OK;
    if (!color_model(h, "bpltv_color_unrolled_gauss_newton", channels, &rc)) return rc;
    return unrolled_gauss_newton_entry(h, "bpltv_color_unrolled_gauss_newton", nullptr, 1, alpha, am, an, pp, cost_out, grad_out, hess_out, channels);
}

int bpltv_u_device(bpltv_t* h, const double** d_u) {
    if (!h || !d_u) return BPLTV_E_ARG;
    if (h->multi)   // (no solve runs: nothing of the multi handle changes, its statistics included)
        return multi_forward0(h, "bpltv_u_device", [&](bpltv_t* c) { return bpltv_u_device(c, d_u); });
    const bool sr = h->last_is_sr && h->sr_has_result;
    if (!sr && !h->has_result) return set_err(h, BPLTV_E_NODATA, "no solve has been run yet");
    *d_u = result_u(h, sr);
    return BPLTV_OK;
}

int bpltv_copy_u_device(bpltv_t* h, double* d_dst) {
    if (!h || !d_dst) return BPLTV_E_ARG;
    if (h->multi) return multi_forward0(h, "bpltv_copy_u_device", [&](bpltv_t* c) { return bpltv_copy_u_device(c, d_dst); });
    const bool sr = h->last_is_sr && h->sr_has_result;
    if (!sr && !h->has_result) return set_err(h, BPLTV_E_NODATA, "no solve has been run yet");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(d_dst, result_u(h, sr), h->tot * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BPLTV_OK;
}

int bpltv_duality_gap(bpltv_t* h, double* gap_out) {
    if (!h || !gap_out) return BPLTV_E_ARG;
    if (h->multi) {
        MultiState& ms = *h->multi;
        const int rc = multi_run(h, [&](int k, bpltv_t* c) { return bpltv_duality_gap(c, gap_out + ms.lo[k]); });
        return rc ? rc : multi_stats(h);
    }
    if (!(h->last_is_sr ? h->sr_has_result : h->has_result)) return set_err(h, BPLTV_E_NODATA, "no solve has been run yet");
    HIPCHK(h, hipSetDevice(h->device));
    double gmax = 0.0;
    const bool sr = h->last_is_sr;
    if (!sr && h->last_channels)
        return set_err(h, BPLTV_E_UNSUPPORTED, "duality gap of a channel-coupled solve (channels = %d): the gap of the coupled model is not implemented", h->last_channels);
    if (!sr && h->last_l1)
        return set_err(h, BPLTV_E_UNSUPPORTED, "duality gap of a TV-L1 solve: its dual has a pointwise constraint the iterate does not meet; the gap is not implemented");
    if (!sr && h->last_kl)
        return set_err(h, BPLTV_E_UNSUPPORTED, "duality gap of a TV-KL solve: the gap of the Kullback-Leibler data term is not implemented");
    const Model model = sr ? MODEL_SR : (h->last_weighted ? MODEL_W : MODEL_TV);
    if (model == MODEL_W && !(h->w_min > 0.0))   // gamma = min w > 0: the weighted model's dual objective divides by w
        return set_err(h, BPLTV_E_UNSUPPORTED, "duality gap of a weighted solve: the dual objective divides by w, every entry must be > 0 (min = %g)", h->w_min);
    int rc = compute_gap(h, dataset_ctx(h, sr), model, sr ? h->sr_result_buf : h->result_buf, gap_out, &gmax);
    if (rc) return rc;
    h->st.last_gap = gmax;
    return BPLTV_OK;
}

int bpltv_grad_fwd(bpltv_t* h, const double* x, double* d1, double* d2) {
    if (!h || !x || !d1 || !d2) return BPLTV_E_ARG;
    if (h->multi)   // one image: the first shard's device
        return multi_run(h, [&](int k, bpltv_t* c) { return k == 0 ? bpltv_grad_fwd(c, x, d1, d2) : BPLTV_OK; });
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = h->npx;
    int rc = ensure(h, &h->d_red, &h->red_cap, 3 * n);
    if (rc) return rc;
    double* b = h->d_red;
    HIPCHK(h, hipMemcpyAsync(b, x, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(grad_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, b, h->M, h->N,
                       b + n, b + 2 * n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d1, b + n, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(d2, b + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BPLTV_OK;
}

int bpltv_grad_fwd_adjoint(bpltv_t* h, const double* y1, const double* y2, double* out) {
    if (!h || !y1 || !y2 || !out) return BPLTV_E_ARG;
    if (h->multi)
        return multi_run(h, [&](int k, bpltv_t* c) { return k == 0 ? bpltv_grad_fwd_adjoint(c, y1, y2, out) : BPLTV_OK; });
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = h->npx;
    int rc = ensure(h, &h->d_red, &h->red_cap, 3 * n);
    if (rc) return rc;
    double* b = h->d_red;
    HIPCHK(h, hipMemcpyAsync(b, y1, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(b + n, y2, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(grad_fwd_T_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, b, b + n, h->M,
                       h->N, b + 2 * n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, b + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BPLTV_OK;
}

int bpltv_gradient(bpltv_t* h, const double* u, const double* ubar, const double* alpha, int am, int an, int reg,
                   const bpltv_params* pp, double* grad_out) {
    if (h) h->has_per_image = false;
    if (!h) return BPLTV_E_ARG;
    if (h->multi) return multi_gradient(h, u, ubar, alpha, am, an, reg, pp, grad_out);
    if (!u || !ubar || !grad_out) return set_err(h, BPLTV_E_ARG, "gradient: null pointer");
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    bpltv_params p = resolve(pp);
    if (int prc = check_params(h, p)) return prc;
    int rc = upload_alpha(h, alpha, false, am, an);
    if (rc) return rc;
    if (!h->d_u2) {
        HIPCHK(h, hipMalloc((void**)&h->d_u2, h->tot * sizeof(double)));
        HIPCHK(h, hipMalloc((void**)&h->d_ubar2, h->tot * sizeof(double)));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_u2, u, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_ubar2, ubar, h->tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = run_gradient(h, h->d_u2, gradient_ctx(h, h->d_ubar2, h->d_partial + 1), reg ? 1 : 0, p);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(grad_out, h->d_partial + 1, sizeof(double) * (size_t)am * an, hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

int bpltv_vjp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp,
              const double* gu, double* grad_f_out, double* grad_alpha_out) {
    return vjp_host(h, u, alpha, am, an, reg, pp, gu, grad_f_out, grad_alpha_out, 1);
}

int bpltv_vjp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg, const bpltv_params* pp,
                     const double* d_gu, double* d_grad_f, double* d_grad_alpha) {
    return vjp_device(h, d_u, d_alpha, am, an, reg, pp, d_gu, d_grad_f, d_grad_alpha, 1);
}

int bpltv_vjp_each(bpltv_t* h, const double* u, const double* alphas, int am, int an, int reg, const bpltv_params* pp,
                   const double* gu, double* grad_f_out, double* grad_alphas_out) {
    return vjp_host(h, u, alphas, am, an, reg, pp, gu, grad_f_out, grad_alphas_out, 1, true);
}
int bpltv_vjp_each_device(bpltv_t* h, const double* d_u, const double* d_alphas, int am, int an, int reg,
                          const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alphas) {
    return vjp_device(h, d_u, d_alphas, am, an, reg, pp, d_gu, d_grad_f, d_grad_alphas, 1, true);
}
int bpltv_jvp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp, int ndir,
              const double* df, const double* dalpha, double* du_out) {
    return jvp_host(h, u, alpha, am, an, reg, pp, ndir, df, dalpha, du_out, false);
}
int bpltv_jvp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg, const bpltv_params* pp,
                     int ndir, const double* d_df, const double* d_dalpha, double* d_du) {
    return jvp_device(h, d_u, d_alpha, am, an, reg, pp, ndir, d_df, d_dalpha, d_du, false);
}
int bpltv_jvp_each(bpltv_t* h, const double* u, const double* alphas, int am, int an, int reg, const bpltv_params* pp, int ndir,
                   const double* df, const double* dalphas, double* du_out) {
    return jvp_host(h, u, alphas, am, an, reg, pp, ndir, df, dalphas, du_out, true);
}
int bpltv_jvp_each_device(bpltv_t* h, const double* d_u, const double* d_alphas, int am, int an, int reg,
                          const bpltv_params* pp, int ndir, const double* d_df, const double* d_dalphas, double* d_du) {
    return jvp_device(h, d_u, d_alphas, am, an, reg, pp, ndir, d_df, d_dalphas, d_du, true);
}
int bpltv_gauss_newton(bpltv_t* h, const double* u, const double* ubar, const double* alpha, int am, int an, int reg,
                       const bpltv_params* pp, double* grad_out, double* hess_out) {
    return gauss_newton(h, u, ubar, alpha, am, an, reg, pp, grad_out, hess_out);
}

int bpltv_sumregs_jvp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp, int ndir,
                      const double* df, const double* dalpha, double* du_out) {
    return jvp_host(h, u, alpha, am, an, reg, pp, ndir, df, dalpha, du_out, false, 3);
}
int bpltv_sumregs_jvp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg, const bpltv_params* pp,
                             int ndir, const double* d_df, const double* d_dalpha, double* d_du) {
    return jvp_device(h, d_u, d_alpha, am, an, reg, pp, ndir, d_df, d_dalpha, d_du, false, 3);
}
int bpltv_sumregs_jvp_each(bpltv_t* h, const double* u, const double* alphas, int am, int an, int reg, const bpltv_params* pp,
                           int ndir, const double* df, const double* dalphas, double* du_out) {
    return jvp_host(h, u, alphas, am, an, reg, pp, ndir, df, dalphas, du_out, true, 3);
}
int bpltv_sumregs_jvp_each_device(bpltv_t* h, const double* d_u, const double* d_alphas, int am, int an, int reg,
                                  const bpltv_params* pp, int ndir, const double* d_df, const double* d_dalphas, double* d_du) {
    return jvp_device(h, d_u, d_alphas, am, an, reg, pp, ndir, d_df, d_dalphas, d_du, true, 3);
}
int bpltv_sumregs_gauss_newton(bpltv_t* h, const double* u, const double* ubar, const double* alpha, int am, int an, int reg,
                               const bpltv_params* pp, double* grad_out, double* hess_out) {
    return gauss_newton(h, u, ubar, alpha, am, an, reg, pp, grad_out, hess_out, 3);
}

int bpltv_sumregs_vjp(bpltv_t* h, const double* u, const double* alpha, int am, int an, int reg, const bpltv_params* pp,
                      const double* gu, double* grad_f_out, double* grad_alpha_out) {
    return vjp_host(h, u, alpha, am, an, reg, pp, gu, grad_f_out, grad_alpha_out, 3);
}

int bpltv_sumregs_vjp_device(bpltv_t* h, const double* d_u, const double* d_alpha, int am, int an, int reg,
                             const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alpha) {
    return vjp_device(h, d_u, d_alpha, am, an, reg, pp, d_gu, d_grad_f, d_grad_alpha, 3);
}

int bpltv_sumregs_vjp_each(bpltv_t* h, const double* u, const double* alphas, int am, int an, int reg, const bpltv_params* pp,
                           const double* gu, double* grad_f_out, double* grad_alphas_out) {
    return vjp_host(h, u, alphas, am, an, reg, pp, gu, grad_f_out, grad_alphas_out, 3, true);
}
int bpltv_sumregs_vjp_each_device(bpltv_t* h, const double* d_u, const double* d_alphas, int am, int an, int reg,
                                  const bpltv_params* pp, const double* d_gu, double* d_grad_f, double* d_grad_alphas) {
    return vjp_device(h, d_u, d_alphas, am, an, reg, pp, d_gu, d_grad_f, d_grad_alphas, 3, true);
}

int bpltv_sweep(bpltv_t* h, const double* alphas, int K, int am, int an, const bpltv_params* pp, double* cost_out,
                double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (!alphas || !cost_out || K < 1) return set_err(h, BPLTV_E_ARG, "sweep: null pointer or K < 1");
    if (am < 1 || an < 1 || am > h->M || an > h->N) return set_err(h, BPLTV_E_ARG, "sweep: bad parameter shape %dx%d", am, an);
    bpltv_params p = resolve(pp);
    // Everything run_pdhg would reject is checked before anything of the handle changes (its buffers included): a
    // rejected sweep leaves the dataset context -- d_alpha, its shape and minimum, the last result -- as it was.
    const size_t npar = (size_t)am * an;
    double amin = 0.0;
    if (int crc = check_alpha_host(h, "sweep: alphas", alphas, (size_t)K * npar, &amin)) return crc;
    if (p.rho != 0.0 && !(amin > 0.0))
        return set_err(h, BPLTV_E_ARG, "sweep: rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", amin);
    if (h->multi) return multi_sweep(h, alphas, K, am, an, pp, cost_out, u_out);
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    if (int prc = check_params(h, p)) return prc;
    if (p.maxiter < 0) return set_err(h, BPLTV_E_ARG, "maxiter < 0");
    const size_t nimg = (size_t)K * h->O;
    {
        Plan pl;
        if (int rc = make_plan(h, p, &pl, (int)nimg)) return rc;
    }
    if ((p.init != 0 || p.order != 0) && h->dtype == 32)
        return set_err(h, BPLTV_E_UNSUPPORTED, "params.init / params.order are implemented for dtype = 64 handles");
    p.check_every = 0;  // the gap kernels address the dataset context only
    if (h->sweep_cap < nimg) {
        drop_graphs(h, DROP_TV);
        for (int s = 0; s < 2; ++s)
            for (int c = 0; c < 3; ++c) {
                if (h->d_sweep[s][c]) HIPCHK(h, hipFree(h->d_sweep[s][c]));
                h->d_sweep[s][c] = nullptr;
                HIPCHK(h, hipMalloc((void**)&h->d_sweep[s][c], nimg * h->npx * sizeof(double)));
            }
        if (h->d_sweep_cost) HIPCHK(h, hipFree(h->d_sweep_cost));
        HIPCHK(h, hipMalloc((void**)&h->d_sweep_cost, nimg * sizeof(double)));
        h->sweep_cap = nimg;
    }
    // the K parameter blocks live in the sweep's own buffer; problem k*O + i uses block k and image i
    if (h->sweep_alpha_cap < K * npar) drop_graphs(h, DROP_TV);   // the sweep's launches hold the old pointer
    int rc = ensure(h, &h->d_sweep_alpha, &h->sweep_alpha_cap, K * npar);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_sweep_alpha, alphas, K * npar * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // the sweep's solve context; nothing of it is committed to the handle
    SolveCtx x;
    for (int sb = 0; sb < 2; ++sb) x.state[sb] = h->d_sweep[sb];
    x.nimg = (int)nimg; x.alpha = h->d_sweep_alpha; x.sweep = true; x.astride = (int)npar;
    x.am = am; x.an = an; x.alpha_min = amin;
    int rb = 0;
    rc = run_pdhg(h, x, p, &rb);
    if (rc) return rc;
    rc = sweep_tail(h, h->d_sweep[rb][0], K, h->d_sweep_cost, cost_out, u_out);
    if (rc) return rc;
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

// The sum-of-regularisers twin of bpltv_sweep: K parameter blocks x O images as K*O problems of run_sr_pdhg, in groups
// of whole parameter blocks that fit the grid (65535 problems) and HBM (14 state planes per problem).  Every problem is
// computed as in any other grouping and its loss reduced on its own, so the result does not depend on the grouping.
// The dataset context (d_sr, d_alpha and the result flags of the last solve) is left as it was.
int bpltv_sumregs_sweep(bpltv_t* h, const double* alphas, int K, int am, int an, const bpltv_params* pp, double* cost_out,
                        double* u_out) {
    if (!h) return BPLTV_E_ARG;
    if (!cost_out) return set_err(h, BPLTV_E_ARG, "sumregs_sweep: null output pointer");
    bpltv_params p = resolve(pp, true);
    // finite and >= 0, and > 0 when rho != 0 -- upload_alpha's and run_sr_pdhg's conditions, before the call changes anything
    if (!alphas || K < 1) return set_err(h, BPLTV_E_ARG, "sumregs_sweep: null pointer or K < 1");
    if (am < 1 || an < 1 || am > h->M || an > h->N) return set_err(h, BPLTV_E_ARG, "sumregs_sweep: bad parameter shape %dx%dx3", am, an);
    double amin = 0.0;
    if (int crc = check_alpha_host(h, "sumregs_sweep: alphas", alphas, (size_t)K * 3 * am * an, &amin)) return crc;
    if (p.rho != 0.0 && !(amin > 0.0))
        return set_err(h, BPLTV_E_ARG, "rho != 0 divides by alpha: every parameter entry must be > 0 (min = %g)", amin);
    if (h->multi) return multi_sweep(h, alphas, K, am, an, pp, cost_out, u_out, 3);
    if (!h->has_data) return set_err(h, BPLTV_E_NODATA, "bpltv_set_data has not been called");
    if (int prc = check_params(h, p)) return prc;
    const int O = h->O;
    if (O > 65535) return set_err(h, BPLTV_E_UNSUPPORTED, "the sum-of-regularisers solve takes at most 65535 images per handle (images are a grid dimension)");
    WallTimer wt;
    HIPCHK(h, hipSetDevice(h->device));
    p.check_every = 0;  // the gap kernels address the dataset context only
    const size_t npx = h->npx, nb = 3 * (size_t)am * an;
    // groups of whole parameter blocks: at most 65535 problems (a grid dimension of the PDHG and loss launches) and what
    // fits the HBM budget (option "sr_sweep_budget_mb", else what is free plus the state already held, minus 2 GB)
    const size_t per_problem = 14 * npx * sizeof(double);
    size_t budget = 0;
    if (h->opt.sr_sweep_budget_mb > 0.0) {
        budget = (size_t)(h->opt.sr_sweep_budget_mb * 1e6);
    } else {
        size_t freeb = 0, totalb = 0;
        (void)hipMemGetInfo(&freeb, &totalb);
        const size_t held = h->srsweep_cap * per_problem, reserve = 2ull << 30;
        budget = freeb + held > reserve ? freeb + held - reserve : 0;
    }
    const size_t kfit = std::min<size_t>(budget / per_problem, 65535) / (size_t)O;
    if (kfit < 1)
        return set_err(h, BPLTV_E_NOMEM, "sumregs_sweep: the state of one parameter block (%d problems of %dx%d) needs %.3f GB of HBM, %.3f GB available",
                       O, h->M, h->N, per_problem * O / 1e9, budget / 1e9);
    const int ng = (int)(((size_t)K + kfit - 1) / kfit);   // equal groups (sizes differ by at most one block: two graphs)
    const int kmax = (K + ng - 1) / ng;
    const size_t pmax = (size_t)kmax * O;
    if (h->srsweep_cap < pmax) {
        drop_graphs(h, DROP_SR);   // captured launches hold the old planes
        h->srsweep_cap = 0;
        for (int sb = 0; sb < 2; ++sb)
            for (int c = 0; c < 7; ++c) {
                if (h->d_srsweep[sb][c]) HIPCHK(h, hipFree(h->d_srsweep[sb][c]));
                h->d_srsweep[sb][c] = nullptr;
            }
        for (int sb = 0; sb < 2; ++sb)
            for (int c = 0; c < 7; ++c) HIPCHK(h, hipMalloc((void**)&h->d_srsweep[sb][c], pmax * npx * sizeof(double)));
        h->srsweep_cap = pmax;
    }
    if (h->srsweep_alpha_cap < kmax * nb) drop_graphs(h, DROP_SR);
    int rc = ensure(h, &h->d_srsweep_alpha, &h->srsweep_alpha_cap, kmax * nb);
    if (rc) return rc;
    rc = ensure(h, &h->d_srsweep_cost, &h->srsweep_cost_cap, pmax);
    if (rc) return rc;
    double pdhg_ms = 0.0, abytes = 0.0;
    int launches = 0, tiles = 0;
    for (int g = 0; g < ng; ++g) {
        const int k0 = (int)(((long)K * g) / ng), k1 = (int)(((long)K * (g + 1)) / ng);
        const int np = (k1 - k0) * O;
        HIPCHK(h, hipMemcpyAsync(h->d_srsweep_alpha, alphas + (size_t)k0 * nb, (size_t)(k1 - k0) * nb * sizeof(double),
                                 hipMemcpyHostToDevice, h->stream));
        // the group's solve context; nothing of it is committed to the handle
        SolveCtx x;
        for (int sb = 0; sb < 2; ++sb) x.state[sb] = h->d_srsweep[sb];
        x.nimg = np; x.alpha = h->d_srsweep_alpha; x.astride = (int)nb;
        x.am = am; x.an = an; x.alpha_min = amin;
        int rb = 0;
        rc = run_sr_pdhg(h, x, p, &rb);
        if (rc) return rc;
        pdhg_ms += h->st.pdhg_ms; launches += h->st.launches; tiles += h->st.tiles; abytes += h->st.algorithmic_bytes;
        rc = sweep_tail(h, h->d_srsweep[rb][0], k1 - k0, h->d_srsweep_cost, cost_out + k0, u_out ? u_out + (size_t)k0 * O * npx : nullptr);
        if (rc) return rc;
    }
    h->st.pdhg_ms = pdhg_ms; h->st.launches = launches; h->st.tiles = tiles; h->st.algorithmic_bytes = abytes;
    h->st.sweep_groups = ng;
    h->st.total_ms = wt.ms();
    return BPLTV_OK;
}

int bpltv_per_image(bpltv_t* h, double* out) {
    if (!h || !out) return BPLTV_E_ARG;
    if (h->multi) {
        if (!h->has_per_image)
            return set_err(h, BPLTV_E_UNSUPPORTED, "per-image pieces exist after evaluate with a scalar or patch parameter only");
        MultiState& ms = *h->multi;
        const size_t W = 1 + (size_t)h->last_am * h->last_an * h->last_slices;
        return multi_run(h, [&](int k, bpltv_t* c) { return bpltv_per_image(c, out + ms.lo[k] * W); });
    }
    if (!h->has_per_image)
        return set_err(h, BPLTV_E_UNSUPPORTED, "per-image pieces exist after evaluate with a scalar or patch parameter only");
    HIPCHK(h, hipSetDevice(h->device));
    const int O = h->O, P = h->last_am * h->last_an * h->last_slices;
    std::vector<double> cost(O), g((size_t)P * O);
    HIPCHK(h, hipMemcpy(cost.data(), h->d_perimg, sizeof(double) * O, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(g.data(), h->d_red, sizeof(double) * P * O, hipMemcpyDeviceToHost));   // [patch][image]
    for (int k = 0; k < O; ++k) {
        out[(size_t)k * (1 + P)] = cost[k];
        for (int q = 0; q < P; ++q) out[(size_t)k * (1 + P) + 1 + q] = g[(size_t)q * O + k];
    }
    return BPLTV_OK;
}

int bpltv_set_option(bpltv_t* h, const char* name, double value) {
    if (!h) return BPLTV_E_ARG;
    if (!name || !std::isfinite(value)) return set_err(h, BPLTV_E_ARG, "set_option: null name or non-finite value");
    if (h->multi) {
        const std::string nm(name);
        if (nm == "sweep_split") {
            const int v = (int)value;
            if (v < 0 || v > 2) return set_err(h, BPLTV_E_ARG, "set_option(sweep_split): 0 automatic, 1 images, 2 parameters");
            h->multi->sweep_split = v;
            return BPLTV_OK;
        }
        if (nm == "tape_checkpoint") {   // (the handle's own copy: bpltv_*_unrolled_tape_doubles reads it)
            if (value != std::floor(value) || value < -1.0 || value > 2147483647.0)
                return set_err(h, BPLTV_E_ARG, "set_option(tape_checkpoint): 0 the full tape, C >= 1 iterations between checkpoints, -1 automatic");
            h->opt.tape_checkpoint = (int)value;
        }
        int rc = multi_run(h, [&](int, bpltv_t* c) { return bpltv_set_option(c, nm.c_str(), value); });
        if (rc == BPLTV_OK && !h->multi->rep.empty())
            rc = rep_run(h, (int)h->multi->rep.size(), [&](int r, bpltv_t* c) { return (r == 0 && h->multi->rep_borrowed0()) ? BPLTV_OK : bpltv_set_option(c, nm.c_str(), value); });
        return rc;
    }
    if (std::string(name) == "sweep_split") return BPLTV_OK;   // single-device handle: nothing to split
    HIPCHK(h, hipSetDevice(h->device));
    const std::string nm(name);
    const int iv = (int)value;
    if (nm == "adjoint_budget_mb") {
        if (value < 0.0) return set_err(h, BPLTV_E_ARG, "set_option(adjoint_budget_mb): must be >= 0");
        h->opt.adjoint_budget_mb = value;
    } else if (nm == "sr_sweep_budget_mb") {
        if (value < 0.0) return set_err(h, BPLTV_E_ARG, "set_option(sr_sweep_budget_mb): must be >= 0");
        h->opt.sr_sweep_budget_mb = value;
    } else if (nm == "sr_force_lu") {
        h->opt.sr_force_lu = iv ? 1 : 0;
    } else if (nm == "tape_checkpoint") {
        if (value != std::floor(value) || value < -1.0 || value > 2147483647.0)
            return set_err(h, BPLTV_E_ARG, "set_option(tape_checkpoint): 0 the full tape, C >= 1 iterations between checkpoints, -1 automatic");
        h->opt.tape_checkpoint = iv;
    } else if (nm == "nd_leaf") {
        if (iv < 0 || iv > 4096) return set_err(h, BPLTV_E_ARG, "set_option(nd_leaf): 0 (default) or 1..4096 pixels");
        if (iv != h->opt.nd_leaf) {   // the trees are built for a leaf size: drop them
            HIPCHK(h, hipStreamSynchronize(h->stream));
            h->nd.release(); h->nd_sr.release(); h->nd_sr_lu.release();
        }
        h->opt.nd_leaf = iv;
    } else if (nm == "nd_wave") {
        h->opt.nd_wave = iv ? 1 : 0;
    } else if (nm == "nd_skinny") {
        h->opt.nd_skinny = iv ? 1 : 0;
    } else if (nm == "nd_skinny_min") {
        h->opt.nd_skinny_min = iv;
    } else if (nm == "nd_skinny2_min") {
        h->opt.nd_skinny2_min = iv;
    } else if (nm == "nd_staged") {
        h->opt.nd_staged = iv ? 1 : 0;
    } else if (nm == "hb_sync" || nm == "hb_single_stream" || nm == "hb_rw") {
        if (nm == "hb_sync" && (iv < 0 || iv > 2)) return set_err(h, BPLTV_E_ARG, "set_option(hb_sync): 0 automatic, 1 events, 2 stream memory operations");
        if (nm == "hb_rw" && iv != 0 && iv != 32 && iv != 128) return set_err(h, BPLTV_E_ARG, "set_option(hb_rw): 0, 32 or 128");
        int& f = nm == "hb_sync" ? h->opt.hb_sync : (nm == "hb_single_stream" ? h->opt.hb_single_stream : h->opt.hb_rw);
        const int nv = nm == "hb_single_stream" ? (iv ? 1 : 0) : iv;
        if (nv != f) {   // the band solvers read these when their workspace is made: drop the workspaces
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (h->band_ready && h->adj_hbm) { h->hb.release(); h->band_ready = false; }
            if (h->sr_band_ready) { h->hb_sr.release(); h->sr_band_ready = false; }
        }
        f = nv;
    } else {
        return set_err(h, BPLTV_E_ARG, "set_option: unknown option '%s'", name);
    }
    return BPLTV_OK;
}

int bpltv_stats(bpltv_t* h, bpltv_stats_t* out) {
    if (!h || !out) return BPLTV_E_ARG;
    *out = h->st;
    return BPLTV_OK;
}

const char* bpltv_last_error(bpltv_t* h) {
    if (!h) return "null handle";
    return h->err.c_str();
}

}  // extern "C"
#pragma GCC visibility pop

#ifdef BPLTV_EXPERIMENTS
// tools/chain_phase.py: the launch-start stamps of the last solve run with params.reserved[3] & 1024 (2 x 4096 ticks of 10 ns)
extern "C" __attribute__((visibility("default"))) int bpltv_debug_tlog(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bpltv::pdhg_tlog), sizeof(long long) * 2 * 4096) == hipSuccess ? 0 : 2;
}
#endif
