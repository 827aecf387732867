# TVLearningFunctionHIP.jl -- the glue of INTEGRATION.md section 1 as a file: include it from
# src/BPLDenoising.jl:31 instead of TVLearningFunctionVec.jl.  It binds libbpltv's C ABI (include/bpltv.h)
# behind the reference's own names; bilevel_learn (src/TRBox.jl) is untouched.
# NOT EXECUTED HERE: Julia is not available in the build image; the same entry points are exercised through
# bpldenoising_amd/_lib.py (ctypes) by the test suite.
# Same exports as src/TVLearningFunctionVec.jl:6
export tv_op_learning_function, denoise, sumregs_learning_function, tv_vjp, sumregs_vjp, tv_jvp, tv_gauss_newton,
       sumregs_jvp, sumregs_gauss_newton, weighted_denoise, weighted_vjp, unrolled_denoise_each, unrolled_vjp_each,
       unrolled_jvp_each, weighted_unrolled_jvp, color_denoise, l1_denoise, kl_denoise, l1_unrolled_jvp, kl_unrolled_jvp

const libbpltv = "libbpltv"            # on LD_LIBRARY_PATH, or an absolute path

# Devices behind the handle: 1 = a single GPU (default); 0 = every visible MI355X (bpltv_create_multi shards the
# images over them and all-reduces [cost, grad...] with RCCL inside the library).  One Julia task drives all of
# them -- the structure of src/TRBox.jl:192-273 does not change.  The default stays 1 until the n > 1 RCCL path
# has run on a multi-GPU node (tests/test_gpu_multi.py holds the device-count-gated checks for that first run).
const BPLTV_NGPUS = parse(Int, get(ENV, "BPLTV_NGPUS", "1"))
# 1: totals bitwise independent of the number of GPUs (all-gather of per-image rows, added in image order)
const BPLTV_DETERMINISTIC = parse(Int, get(ENV, "BPLTV_DETERMINISTIC", "0"))
# The choices of the PDHG loop the reference does not pin (VariationalImaging.op_denoise_pdps is not in the repo):
# set these if your installed VariationalImaging starts from x0 = 0, takes the dual step first, or estimates the
# operator norm differently (include/bpltv.h: bpltv_params.init / order / opnorm; 0 = the restatement).
const BPLTV_INIT = parse(Int, get(ENV, "BPLTV_INIT", "0"))
const BPLTV_ORDER = parse(Int, get(ENV, "BPLTV_ORDER", "0"))
const BPLTV_OPNORM = parse(Float64, get(ENV, "BPLTV_OPNORM", "0"))

# struct bpltv_params (include/bpltv.h) -- field order and types must match
struct BpltvParams
    rho::Cdouble; tau0::Cdouble; sigma0::Cdouble
    accel::Cint; maxiter::Cint
    delta_t::Cdouble
    check_every::Cint
    gap_tol::Cdouble
    tile_iters::Cint; use_graph::Cint
    kappa_cap::Cdouble
    refine::Cint
    deterministic::Cint
    reserved::NTuple{5,Cint}
    init::Cint            # 0: x0 = f; 1: x0 = 0                  (unpinned choices of op_denoise_pdps,
    order::Cint           # 0: primal step first; 1: dual first    DESIGN.md 2.3; 0 = the restatement)
    opnorm::Cdouble       # operator-norm estimate L; 0 = sqrt(8)
end

mutable struct BpltvHandle
    ptr::Ptr{Cvoid}
    M::Int; N::Int; O::Int
    # The dataset currently resident on the GPUs.  The arrays themselves are kept (not their objectid): a
    # reference held here keeps them alive, so a later dataset cannot be allocated at the same address and
    # pass for this one after a GC; identity is compared with `===`.
    ū::Union{Nothing,Array{Float64,3}}
    f::Union{Nothing,Array{Float64,3}}
    fingerprint::Tuple{Float64,Float64}   # (sum(ū), sum(f)) at upload time: catches in-place edits
end

function bpltv_check(h::BpltvHandle, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:bpltv_last_error, libbpltv), Cstring, (Ptr{Cvoid},), h.ptr))
    error("libbpltv error $rc: $msg")  # reference behaviour: exceptions propagate
end

function BpltvHandle(M, N, O; ngpus = BPLTV_NGPUS)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:bpltv_create_multi, libbpltv), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
               p, M, N, O, ngpus, 64)
    h = BpltvHandle(p[], M, N, O, nothing, nothing, (NaN, NaN))
    finalizer(x -> ccall((:bpltv_destroy, libbpltv), Cint, (Ptr{Cvoid},), x.ptr), h)
    bpltv_check(h, rc)
    return h
end

function default_params(; kwargs...)
    r = Ref{BpltvParams}()
    ccall((:bpltv_default_params, libbpltv), Cint, (Ref{BpltvParams},), r)
    p = r[]
    # the reference's NamedTuple keys (src/TVLearningFunctionVec.jl:33-43); others are ignored
    get_(k, d) = haskey(kwargs, k) ? kwargs[k] : d
    return BpltvParams(get_(:ρ, p.rho), get_(:τ₀, p.tau0), get_(:σ₀, p.sigma0),
                       get_(:accel, p.accel != 0) ? 1 : 0, get_(:maxiter, p.maxiter),
                       get_(:Δt, p.delta_t), p.check_every, p.gap_tol, p.tile_iters, p.use_graph,
                       p.kappa_cap, p.refine, BPLTV_DETERMINISTIC, p.reserved, BPLTV_INIT, BPLTV_ORDER, BPLTV_OPNORM)
end

const _handle = Ref{Union{Nothing,BpltvHandle}}(nothing)

# One handle per dataset: bilevel_learn passes the same `ds` to every evaluation
# (src/TRBox.jl:210,227), so the images are uploaded once.  A different array object, or the same object
# with edited content, is uploaded again.
function handle_for(ū::Array{Float64,3}, f::Array{Float64,3})
    M, N, O = size(f)
    h = _handle[]
    if h === nothing || (h.M, h.N, h.O) != (M, N, O)
        h = BpltvHandle(M, N, O); _handle[] = h
    end
    fp = (sum(ū), sum(f))
    if !(h.ū === ū && h.f === f && h.fingerprint == fp)
        GC.@preserve ū f bpltv_check(h, ccall((:bpltv_set_data, libbpltv), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h.ptr, ū, f))
        h.ū = ū; h.f = f; h.fingerprint = fp
    end
    return h
end

alpha_arg(x::Real) = (Float64[x], 1, 1)
alpha_arg(x::AbstractVector) = (Vector{Float64}(x), length(x), 1)
alpha_arg(x::AbstractMatrix) = (Matrix{Float64}(x), size(x, 1), size(x, 2))   # column major m x n

# src/TVLearningFunctionVec.jl:14-27
function tv_op_learning_function(x, data, Δ; Δt = 1e-6, kwargs...)
    ū, f = data[1], data[2]
    h = handle_for(ū, f)
    a, am, an = alpha_arg(x)
    u = similar(f); cost = Ref{Cdouble}(0); grad = zeros(am, an)
    p = Ref(default_params(; Δt = Δt, kwargs...))
    GC.@preserve a u grad bpltv_check(h, ccall((:bpltv_evaluate, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ref{BpltvParams}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, am, an, Δ, p, u, cost, grad))
    # grad has the type of x: Float64 for scalar x (src/TRBox.jl:37-39,167,237)
    return u, cost[], x isa Real ? grad[1] : reshape(grad, size(x))
end

# src/TVLearningFunctionVec.jl:45-70 (op must be FwdGradientOp(); it is the only operator on this path)
function denoise(data::Array{Float64,3}, x, op::LinOp; kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a u bpltv_check(h, ccall((:bpltv_denoise, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, a, am, an, p, u))
    return u
end

# src/BPLDenoising.jl:41-82
TVDenoise(data, parameter; visualize = false) = denoise(data, parameter, FwdGradientOp(); maxiter = 10000)

# src/SumRegsLearningFunction.jl:8-36 -- x::Vector (3 weights: forward, backward, centred TV) or x::Array{T,3} (m x n x 3).
# The C ABI takes the three slices one after the other, which is exactly Julia's column-major memory of x.
function sumregs_learning_function(x::Union{AbstractVector{Float64},AbstractArray{Float64,3}}, data, Δ; Δt = 1e-3)
    ū, f = data[1], data[2]
    h = handle_for(ū, f)
    a = Array{Float64}(x)
    am, an = x isa AbstractVector ? (1, 1) : (size(x, 1), size(x, 2))
    u = similar(f); cost = Ref{Cdouble}(0); grad = zeros(size(a))
    r = Ref{BpltvParams}()
    ccall((:bpltv_sumregs_default_params, libbpltv), Cint, (Ref{BpltvParams},), r)
    d = r[]
    p = Ref(BpltvParams(d.rho, d.tau0, d.sigma0, d.accel, d.maxiter, Δt, d.check_every, d.gap_tol, d.tile_iters,
                        d.use_graph, d.kappa_cap, d.refine, BPLTV_DETERMINISTIC, d.reserved, BPLTV_INIT, BPLTV_ORDER, BPLTV_OPNORM))
    GC.@preserve a u grad bpltv_check(h, ccall((:bpltv_sumregs_evaluate, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ref{BpltvParams}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, am, an, Δ, p, u, cost, grad))
    return u, cost[], grad
end

# generate_cost / generate_2d_cost, src/BPLDenoising.jl:92-111,136-158: cost(alpha_k) = L2CostFunction(TVDenoise(f, alpha_k), true)
# for K parameters (a Vector of scalars, or an m x n x K array of parameter matrices) as ONE bpltv_sweep call.  Over several
# GPUs (BPLTV_NGPUS) the library splits the images or -- a one-image dataset, the default num_samples = 1 of :313 -- the K
# parameter blocks over replicas of the dataset; the costs are bitwise those of one GPU.
function generate_cost_sweep(data, parameters; maxiter = 10000)
    ū, f = data[1], data[2]
    h = handle_for(ū, f)
    a = Array{Float64}(parameters)
    am, an, K = ndims(a) == 1 ? (1, 1, length(a)) : (size(a, 1), size(a, 2), size(a, 3))
    costs = zeros(K)
    p = Ref(default_params(; maxiter = maxiter))
    GC.@preserve a costs bpltv_check(h, ccall((:bpltv_sweep, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, K, am, an, p, costs, C_NULL))
    return costs
end

# generate_cost with denoise_function = sumregs_denoise (src/BPLDenoising.jl:92-111, src/SumRegsLearningFunction.jl:38-85):
# K weight triples (a 3 x K matrix) or K m x n x 3 parameter arrays (an m x n x 3 x K array; block k is x_k's column-major
# memory, as sumregs_learning_function passes it) as ONE bpltv_sumregs_sweep call, maxiter = 5000 as sumregs_denoise.
# Over several GPUs the images or the parameter blocks are split as in generate_cost_sweep.
function generate_sumregs_cost_sweep(data, parameters; maxiter = 5000)
    ū, f = data[1], data[2]
    h = handle_for(ū, f)
    a = Array{Float64}(parameters)
    am, an, K = ndims(a) == 2 ? (1, 1, size(a, 2)) : (size(a, 1), size(a, 2), size(a, 4))
    costs = zeros(K)
    r = Ref{BpltvParams}()
    ccall((:bpltv_sumregs_default_params, libbpltv), Cint, (Ref{BpltvParams},), r)
    d = r[]
    p = Ref(BpltvParams(d.rho, d.tau0, d.sigma0, d.accel, maxiter, d.delta_t, d.check_every, d.gap_tol, d.tile_iters,
                        d.use_graph, d.kappa_cap, d.refine, BPLTV_DETERMINISTIC, d.reserved, BPLTV_INIT, BPLTV_ORDER, BPLTV_OPNORM))
    GC.@preserve a costs bpltv_check(h, ccall((:bpltv_sumregs_sweep, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, K, am, an, p, costs, C_NULL))
    return costs
end

# Vector-Jacobian product of u = denoise(f, α) for a cotangent ḡ = dL/du of any upper-level loss L (include/bpltv.h,
# bpltv_vjp): (dL/df, dL/dα) from one adjoint solve.  ḡ = u - ū gives tv_op_learning_function's gradient bit for bit;
# reg = true is its gradient_reg branch (Δ <= Δt).  The dataset is not used: any handle of u's size will do.
function tv_vjp(h::BpltvHandle, u::Array{Float64,3}, α, ḡ::Array{Float64,3}; reg = false, kwargs...)
    a, am, an = alpha_arg(α)
    gf = similar(u); ga = zeros(am, an)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u a ḡ gf ga bpltv_check(h, ccall((:bpltv_vjp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, a, am, an, reg ? 1 : 0, p, ḡ, gf, ga))
    return gf, α isa Real ? ga[1] : reshape(ga, size(α))
end

# Per-pixel data-fidelity weight (include/bpltv.h, bpltv_weighted_denoise): min_u 0.5 Σ w (u - f)^2 + Σ α |∇u| for a mask
# (w ∈ {0, 1}: inpainting), a known noise variance per pixel (w = 1/σ^2) or a learnable fidelity map.  w >= 0: an M x N
# matrix (one plane for every image) or an M x N x O array (one per image).  w = 1 everywhere is denoise(data, x, op).
function weighted_denoise(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}}; kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a u bpltv_check(h, ccall((:bpltv_weighted_denoise, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, u))
    return u
end

# TV-L1 (include/bpltv.h, bpltv_lone_denoise): min_u Σ w |u - f| + Σ α |∇u|, the model for salt-and-pepper noise, outliers and dead
# pixels -- an isolated outlier is removed exactly and the rest keeps its contrast.  w as in weighted_denoise; maxiter iterations.
function l1_denoise(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}}; kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a u bpltv_check(h, ccall((:bpltv_lone_denoise, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, u))
    return u
end

# TV-KL (include/bpltv.h, bpltv_kl_denoise): min_u Σ w (u - f log u) + Σ α |∇u| over u ≥ 0, the model for Poisson noise (photon
# counts).  data must be finite and ≥ 0, zero counts allowed; w as in weighted_denoise; maxiter iterations.
function kl_denoise(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}}; kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a u bpltv_check(h, ccall((:bpltv_kl_denoise, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, u))
    return u
end

# Its vector-Jacobian product (bpltv_weighted_vjp): (dL/df, dL/dα, dL/dw) from one adjoint solve of (diag(w) + K) p = ḡ, in the
# `gradient` linearisation; dL/dw has the shape of w (an M x N weight: summed over the images).  Every w must be > 0.
function weighted_vjp(h::BpltvHandle, u::Array{Float64,3}, f::Array{Float64,3}, α, w::Union{Matrix{Float64},Array{Float64,3}},
                      ḡ::Array{Float64,3}; kwargs...)
    a, am, an = alpha_arg(α)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    gf = similar(u); ga = zeros(am, an); gw = similar(w)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u f w a ḡ gf ga gw bpltv_check(h, ccall((:bpltv_weighted_vjp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), h.ptr, u, f, w, wo, a, am, an, p, ḡ, gf, ga, gw))
    return gf, (α isa Real ? ga[1] : reshape(ga, size(α))), gw
end

# Forward mode through the weighted PDHG iterations (include/bpltv.h, bpltv_weighted_unrolled_jvp): du of the maxiter-step map
# u = weighted_denoise(data, x, w) for one direction (df, dα, dw), by a tangent sweep that records no tape and -- unlike
# weighted_vjp -- needs no w > 0, so a mask has sensitivities.  df: nothing or M x N x O; dα: nothing, a number for a scalar x
# or shaped like x; dw: nothing or shaped like w; not all three nothing.  Returns (du, u) with u the primal result.  The step
# table (γ = min w) is held fixed.
function weighted_unrolled_jvp(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}};
                               df = nothing, dα = nothing, dw = nothing, kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    df === nothing && dα === nothing && dw === nothing && error("weighted_unrolled_jvp: df, dα and dw are all nothing")
    dw === nothing || size(dw) == size(w) || error("weighted_unrolled_jvp: dw must have the shape of w")
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dα === nothing ? C_NULL : (dα isa Real ? [Float64(dα)] : Array{Float64}(dα))
    tw = dw === nothing ? C_NULL : Array{Float64}(dw)
    du = similar(data); u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a tf ta tw du u bpltv_check(h, ccall((:bpltv_weighted_unrolled_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, 1, tf, ta, tw, du, u))
    return du, u
end

# Forward mode through the TV-L1 iterations (include/bpltv.h, bpltv_lone_unrolled_jvp): du of the maxiter-step map
# u = l1_denoise(data, x, w) for one direction (df, dα, dw), by a tangent sweep that records no tape; arguments and result as
# weighted_unrolled_jvp's.  A pixel the threshold holds at f moves with f alone.
function l1_unrolled_jvp(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}};
                         df = nothing, dα = nothing, dw = nothing, kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    df === nothing && dα === nothing && dw === nothing && error("l1_unrolled_jvp: df, dα and dw are all nothing")
    dw === nothing || size(dw) == size(w) || error("l1_unrolled_jvp: dw must have the shape of w")
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dα === nothing ? C_NULL : (dα isa Real ? [Float64(dα)] : Array{Float64}(dα))
    tw = dw === nothing ? C_NULL : Array{Float64}(dw)
    du = similar(data); u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a tf ta tw du u bpltv_check(h, ccall((:bpltv_lone_unrolled_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, 1, tf, ta, tw, du, u))
    return du, u
end

# Forward mode through the TV-KL iterations (include/bpltv.h, bpltv_kl_unrolled_jvp): du of the maxiter-step map
# u = kl_denoise(data, x, w) for one direction (df, dα, dw), by a tangent sweep that records no tape; arguments and result as
# weighted_unrolled_jvp's.  data must be finite and >= 0; a pixel clamped at zero passes nothing.
function kl_unrolled_jvp(data::Array{Float64,3}, x, w::Union{Matrix{Float64},Array{Float64,3}};
                         df = nothing, dα = nothing, dw = nothing, kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(x)
    wo = ndims(w) == 2 ? 1 : size(w, 3)
    df === nothing && dα === nothing && dw === nothing && error("kl_unrolled_jvp: df, dα and dw are all nothing")
    dw === nothing || size(dw) == size(w) || error("kl_unrolled_jvp: dw must have the shape of w")
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dα === nothing ? C_NULL : (dα isa Real ? [Float64(dα)] : Array{Float64}(dα))
    tw = dw === nothing ? C_NULL : Array{Float64}(dw)
    du = similar(data); u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve w a tf ta tw du u bpltv_check(h, ccall((:bpltv_kl_unrolled_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}), h.ptr, w, wo, a, am, an, p, 1, tf, ta, tw, du, u))
    return du, u
end

# Jacobian-vector product of u = denoise(f, α) (include/bpltv.h, bpltv_jvp): du for the tangents (df, dα), the linear map
# whose transpose tv_vjp computes, so dot(ḡ, du) == dot(gf, df) + dot(gα, dα).  df: nothing or an M x N x O array, or
# M x N x O x K for K directions solved against one factorisation; dα: nothing, or shaped like α (a number for a scalar α),
# or with a trailing dimension K (a K-vector for a scalar α).  Returns du shaped like df (like u for one direction).
function tv_jvp(h::BpltvHandle, u::Array{Float64,3}, α; df = nothing, dα = nothing, reg = false, kwargs...)
    a, am, an = alpha_arg(α)
    df === nothing && dα === nothing && error("tv_jvp: df and dα are both nothing")
    K = df !== nothing ? size(df, 4) : (dα isa Real ? 1 : div(length(dα), am * an))
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dα === nothing ? C_NULL : (dα isa Real ? Float64[dα] : Array{Float64}(dα))
    du = zeros(size(u)..., K)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u a tf ta du bpltv_check(h, ccall((:bpltv_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, a, am, an, reg ? 1 : 0, p, K, tf, ta, du))
    return K == 1 && (df === nothing || ndims(df) == 3) ? du[:, :, :, 1] : du
end

# Gauss-Newton model of 0.5||u(α) - ū||^2 (include/bpltv.h, bpltv_gauss_newton): (g, H) with g = J'(u - ū) shaped like α
# and H = J'J (P x P, P = length(α) <= 16, in α's column-major order) from the P columns du/dα_j, solved against one
# factorisation -- a second-order model for the trust region of src/TRBox.jl, whose own model Hessian is B = 0.1 or L-BFGS.
function tv_gauss_newton(h::BpltvHandle, u::Array{Float64,3}, ū::Array{Float64,3}, α; reg = false, kwargs...)
    a, am, an = alpha_arg(α)
    P = am * an
    g = zeros(am, an); H = zeros(P, P)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u ū a g H bpltv_check(h, ccall((:bpltv_gauss_newton, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, ū, a, am, an, reg ? 1 : 0, p, g, H))
    return (α isa Real ? g[1] : reshape(g, size(α))), H
end

# One parameter per image through the PDHG iterations (include/bpltv.h, bpltv_unrolled_denoise_each / _vjp_each / _jvp_each):
# what a network that predicts α per sample needs in front of a fixed, small maxiter.  αs: an O-vector (one scalar per
# image) or an m x n x O array (block k = αs[:, :, k], column major, as the library reads it).
alphas_arg(x::AbstractVector) = (Vector{Float64}(x), 1, 1)
alphas_arg(x::AbstractArray{<:Real,3}) = (Array{Float64,3}(x), size(x, 1), size(x, 2))

# u[:, :, k] = denoise(data[:, :, k], αs[k]) by exactly maxiter iterations; records the handle's tape, per image.
function unrolled_denoise_each(data::Array{Float64,3}, αs; kwargs...)
    h = handle_for(data, data)
    a, am, an = alphas_arg(αs)
    length(a) == am * an * size(data, 3) || error("unrolled_denoise_each: one parameter block per image")
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a u bpltv_check(h, ccall((:bpltv_unrolled_denoise_each, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, a, am, an, p, u))
    return h, u
end

# (dL/df, dL/dαs) of the maxiter-step map by a reverse sweep over the handle's per-image tape: same h, αs and params as the
# solve.  dL/dαs has the shape of αs; block k is image k's term alone.
function unrolled_vjp_each(h::BpltvHandle, αs, ḡ::Array{Float64,3}; kwargs...)
    a, am, an = alphas_arg(αs)
    gf = similar(ḡ); ga = zeros(size(a))
    p = Ref(default_params(; kwargs...))
    GC.@preserve a ḡ gf ga bpltv_check(h, ccall((:bpltv_unrolled_vjp_each, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, am, an, p, ḡ, gf, ga))
    return gf, ga
end

# du of the maxiter-step map of the handle's dataset for one direction (df, dαs): df nothing or M x N x O, dαs nothing or
# shaped like αs; returns (du, u) with u the primal result.
function unrolled_jvp_each(h::BpltvHandle, αs; df = nothing, dαs = nothing, kwargs...)
    a, am, an = alphas_arg(αs)
    df === nothing && dαs === nothing && error("unrolled_jvp_each: df and dαs are both nothing")
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dαs === nothing ? C_NULL : Array{Float64}(dαs)
    du = zeros(h.M, h.N, h.O); u = zeros(h.M, h.N, h.O)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a tf ta du u bpltv_check(h, ccall((:bpltv_unrolled_jvp_each, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, a, am, an, p, 1, tf, ta, du, u))
    return du, u
end

# Channel-coupled (vectorial) TV of colour images (include/bpltv.h, bpltv_color_denoise): data is M x N x (C*B), colour image b
# owns the planes (b-1)*C+1 ... b*C, and the channels of a pixel share one projection.  α: a scalar or an m x n matrix, shared
# by the batch and the channels.  bpltv_color_unrolled_denoise / bpltv_color_unrolled_vjp take the same leading `channels`.
function color_denoise(data::Array{Float64,3}, α, channels::Integer; kwargs...)
    h = handle_for(data, data)
    a, am, an = alpha_arg(α)
    u = similar(data)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a u bpltv_check(h, ccall((:bpltv_color_denoise, libbpltv), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}), h.ptr, channels, a, am, an, p, u))
    return u
end

# Forward mode through the channel-coupled iterations (include/bpltv.h, bpltv_color_unrolled_jvp): du of the maxiter-step map
# of the handle's dataset for one direction (df, dα): df nothing or M x N x (C*B), dα nothing or shaped like α; returns
# (du, u) with u = color_denoise's result.  No tape is read: the transpose of bpltv_color_unrolled_vjp.
function color_unrolled_jvp(h::BpltvHandle, α, channels::Integer; df = nothing, dα = nothing, kwargs...)
    a, am, an = alpha_arg(α)
    df === nothing && dα === nothing && error("color_unrolled_jvp: df and dα are both nothing")
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dα === nothing ? C_NULL : (dα isa Real ? [Float64(dα)] : Array{Float64}(dα))
    du = zeros(h.M, h.N, h.O); u = zeros(h.M, h.N, h.O)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a tf ta du u bpltv_check(h, ccall((:bpltv_color_unrolled_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, channels, a, am, an, p, 1, tf, ta, du, u))
    return du, u
end

# The same with everything resident in HBM (bpltv_color_unrolled_jvp_device): raw device addresses, ndir directions,
# direction-major; d_df or d_dα may be C_NULL (not both), d_u may be C_NULL.
function color_unrolled_jvp_device(h::BpltvHandle, channels::Integer, d_α::Ptr{Cvoid}, am::Integer, an::Integer, d_df::Ptr{Cvoid},
                                   d_dα::Ptr{Cvoid}, d_du::Ptr{Cvoid}, d_u::Ptr{Cvoid} = C_NULL; ndir::Integer = 1, kwargs...)
    p = Ref(default_params(; kwargs...))
    bpltv_check(h, ccall((:bpltv_color_unrolled_jvp_device, libbpltv), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        h.ptr, channels, d_α, am, an, p, ndir, d_df, d_dα, d_du, d_u))
    return nothing
end

# Gauss-Newton model of the maxiter-step loss 0.5||u_K(α) - ū||^2 of the channel-coupled solve on the handle's dataset
# (bpltv_color_unrolled_gauss_newton): (cost, g, H) with g = J'(u_K - ū) shaped like α and H = J'J (P x P, P = length(α) <= 16,
# in α's column-major order) from P tangent sweeps -- the model the trust region of src/TRBox.jl consumes.
function color_unrolled_gauss_newton(h::BpltvHandle, α, channels::Integer; kwargs...)
    a, am, an = alpha_arg(α)
    P = am * an
    cost = Ref(0.0); g = zeros(am, an); H = zeros(P, P)
    p = Ref(default_params(; kwargs...))
    GC.@preserve a g H bpltv_check(h, ccall((:bpltv_color_unrolled_gauss_newton, libbpltv), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint, Ref{BpltvParams}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, channels, a, am, an, p, cost, g, H))
    return cost[], (α isa Real ? g[1] : reshape(g, size(α))), H
end

# The same for u = sumregs_denoise(f, x) (include/bpltv.h, bpltv_sumregs_vjp): x a 3-vector or an m x n x 3 array, passed
# as its column-major memory as in sumregs_learning_function; dL/dx has the shape of x.  ḡ = u - ū gives
# sumregs_learning_function's gradient bit for bit; reg = true is its sumregs_gradient_reg branch (Δ <= Δt).
function sumregs_vjp(h::BpltvHandle, u::Array{Float64,3}, x::Union{AbstractVector{Float64},AbstractArray{Float64,3}},
                     ḡ::Array{Float64,3}; reg = false, kwargs...)
    a = Array{Float64}(x)
    am, an = x isa AbstractVector ? (1, 1) : (size(x, 1), size(x, 2))
    gf = similar(u); ga = zeros(size(a))
    p = Ref(default_params(; kwargs...))
    GC.@preserve u a ḡ gf ga bpltv_check(h, ccall((:bpltv_sumregs_vjp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, a, am, an, reg ? 1 : 0, p, ḡ, gf, ga))
    return gf, ga
end

# Jacobian-vector product of u = sumregs_denoise(f, x) (include/bpltv.h, bpltv_sumregs_jvp): du for the tangents (df, dx),
# the linear map whose transpose sumregs_vjp computes, so dot(ḡ, du) == dot(gf, df) + dot(gx, dx) -- also for reg = true
# with an m x n x 3 parameter, whose row-scaled system the library solves transposed.  df: nothing or an M x N x O array, or
# M x N x O x K for K directions against one factorisation; dx: nothing, or shaped like x, or with a trailing dimension K.
function sumregs_jvp(h::BpltvHandle, u::Array{Float64,3}, x::Union{AbstractVector{Float64},AbstractArray{Float64,3}};
                     df = nothing, dx = nothing, reg = false, kwargs...)
    a = Array{Float64}(x)
    am, an = x isa AbstractVector ? (1, 1) : (size(x, 1), size(x, 2))
    df === nothing && dx === nothing && error("sumregs_jvp: df and dx are both nothing")
    K = df !== nothing ? size(df, 4) : div(length(dx), length(a))
    tf = df === nothing ? C_NULL : Array{Float64}(df)
    ta = dx === nothing ? C_NULL : Array{Float64}(dx)
    du = zeros(size(u)..., K)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u a tf ta du bpltv_check(h, ccall((:bpltv_sumregs_jvp, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, a, am, an, reg ? 1 : 0, p, K, tf, ta, du))
    return K == 1 && (df === nothing || ndims(df) == 3) ? du[:, :, :, 1] : du
end

# Gauss-Newton model of 0.5||u(x) - ū||^2 for the sum-of-regularisers model (include/bpltv.h, bpltv_sumregs_gauss_newton):
# (g, H) with g = J'(u - ū) shaped like x and H = J'J (P x P, P = length(x) <= 16, in x's column-major order) from one
# factorisation -- the 3 x 3 model of the learning problem x = [a1; a2; a3] of src/SumRegsLearningFunction.jl:8, or the
# 12 x 12 one of a 2 x 2 x 3 patch, for a trust-region step in place of BFGS.
function sumregs_gauss_newton(h::BpltvHandle, u::Array{Float64,3}, ū::Array{Float64,3},
                              x::Union{AbstractVector{Float64},AbstractArray{Float64,3}}; reg = false, kwargs...)
    a = Array{Float64}(x)
    am, an = x isa AbstractVector ? (1, 1) : (size(x, 1), size(x, 2))
    P = length(a)
    g = zeros(size(a)); H = zeros(P, P)
    p = Ref(default_params(; kwargs...))
    GC.@preserve u ū a g H bpltv_check(h, ccall((:bpltv_sumregs_gauss_newton, libbpltv), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ref{BpltvParams}, Ptr{Cdouble}, Ptr{Cdouble}),
        h.ptr, u, ū, a, am, an, reg ? 1 : 0, p, g, H))
    return g, H
end

# test / measurement aids of a handle (include/bpltv.h, bpltv_set_option), e.g. set_option(h, "sweep_split", 2)
set_option(h::BpltvHandle, name::String, value::Real) =
    bpltv_check(h, ccall((:bpltv_set_option, libbpltv), Cint, (Ptr{Cvoid}, Cstring, Cdouble), h.ptr, name, value))
