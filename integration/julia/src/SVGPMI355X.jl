# SVGPMI355X.jl — the reference-side binding of libsvgp_mi355x.so (include/svgp_mi355x.h).
#
# What a maintainer of ApproximateGPs.jl adds so that `elbo` / `approx_lml` / `posterior` and the predictive API of a
# `SparseVariationalApproximation` run on an MI355X WITHOUT any change at the call sites — including under Zygote
# (examples/a-regression/script.jl:136-141,188-194, examples/b-classification/script.jl:132-142,
# test/SparseVariationalApproximationModule.jl:163-175) and for `mean / var / cov / mean_and_var / mean_and_cov /
# cov(x, y)` (SVA:208-264):
#
#   1. src/mi355x_hooks.jl (the hook functions with their do-nothing fallbacks), included before the SVA module,
#   2. this file, included after it (it needs the SVA types), and
#   3. the one-line hooks of integration/julia/ApproximateGPs_hooks.patch at the top of the reference methods
#      (`r = MI355XHooks.try_elbo(...); r === nothing || return r`).
#
# A hook returns `nothing` whenever the library is absent, switched off (`SVGPMI355X.enable!(false)`) or the model is
# outside what the library supports (status SVGP_UNSUPPORTED, exotic kernels / transforms / likelihoods / element types),
# and the reference's own body then runs unchanged.  No method is shadowed, nothing is `invoke`d.
#
# AD: `try_elbo` carries a `ChainRulesCore.rrule` whose pullback returns STRUCTURAL tangents for `sva` (kernel variance,
# inverse lengthscales, inducing inputs, constant mean, mean(q), the Cholesky factor of cov(q)) and for the likelihood
# parameter, and for the data inputs `lfx.fx.x` (what a learned feature map in front of the GP back-propagates: x = NN(θ)(raw)),
# from ONE svgp_elbo_grad_inputs call (svgp_elbo_grad_ext_inputs for a likelihood evaluated here).  When the hook declines, its
# rrule returns `nothing` with zero tangents and Zygote differentiates the reference body as before.  Gradients with respect to
# the observations `y` and the jitter `fz.Σy` are not computed by the library (zero tangents).
#
# NOT EXECUTED IN THIS REPOSITORY: the build image has no Julia.  The identical C symbols, struct layouts and status
# conventions are exercised by the Python ctypes mirror (approximategps.jl_amd/approxgp/_ffi.py) that tests/ call;
# tests/test_abi_cpu.py pins the struct sizes / offsets asserted in integration/julia/test/runtests.jl.
#
# File:line references are to the reference repository (SVA = src/SparseVariationalApproximationModule.jl).
module SVGPMI355X

using AbstractGPs, KernelFunctions, GPLikelihoods, LinearAlgebra, Distributions
using ChainRulesCore
using FillArrays: Fill
using PDMats: PDMat, ScalMat
import Libdl

# `..` = ApproximateGPs: this file is included from src/ApproximateGPs.jl after mi355x_hooks.jl and the SVA module
using ..MI355XHooks
using ..SparseVariationalApproximationModule: SparseVariationalApproximation, Centered, NonCentered
using ..ApproximateGPs: _chol_lower, _chol_cov, ApproxPosteriorGP

const lib = get(ENV, "SVGP_MI355X_LIB", "libsvgp_mi355x.so")
const FT = Union{Float32,Float64}
const ENABLED = Ref(true)
"Switch every hook off (they return `nothing`) or back on; the reference's pure-Julia bodies then run."
enable!(on::Bool) = (ENABLED[] = on)

# ---------------------------------------------------------------------------------------------------------
# C structs, field for field (include/svgp_mi355x.h; sizes 104 / 64 / 56 bytes, checked in test/runtests.jl)
# ---------------------------------------------------------------------------------------------------------
struct ModelDesc                      # svgp_model_desc
    dtype::Int32; kernel::Int32; parametrization::Int32; likelihood::Int32
    quadrature_n::Int32; layout_z::Int32; neg_var_policy::Int32; d::Int32
    M::Int64; variance::Float64; inv_lengthscale::Ptr{Float64}
    mean_const::Float64; jitter::Float64; lik_sigma2::Float64
    z::Ptr{Cvoid}; m::Ptr{Cvoid}; Lq::Ptr{Cvoid}
end

mutable struct Terms                  # svgp_terms
    elbo::Float64; expectation::Float64; kl::Float64; scale::Float64; logdet_kuu::Float64
    n_points::Int64; n_neg_var::Int64; chol_info::Int32; reserved::Int32
    Terms() = new(0, 0, 0, 0, 0, 0, 0, 0, 0)
end

mutable struct Grads                  # svgp_grads
    variance::Float64; lik_sigma2::Float64; mean_const::Float64
    inv_lengthscale::Ptr{Float64}; z::Ptr{Cvoid}; m::Ptr{Cvoid}; Lq::Ptr{Cvoid}
end

struct InputGrad                      # svgp_input_grad (24 bytes): d elbo / d x, element (f, j) at x[f * ld + j]
    x::Ptr{Cvoid}
    ld::Int64
    on_device::Int32
    reserved::Int32
end

struct PointMean                      # svgp_point_mean (16 bytes): the batch's prior mean offsets mux
    mu::Ptr{Cvoid}
    on_device::Int32
    reserved::Int32
end

struct PointMeanGrad                  # svgp_point_mean_grad (16 bytes): d elbo / d mux
    mu_bar::Ptr{Cvoid}
    on_device::Int32
    reserved::Int32
end

struct PointNoise                     # svgp_point_noise (16 bytes): the batch's per-point noise variances s (added to lik_sigma2)
    s::Ptr{Cvoid}
    on_device::Int32
    reserved::Int32
end

struct PointNoiseGrad                 # svgp_point_noise_grad (16 bytes): d bound / d sigma_j^2
    s_bar::Ptr{Cvoid}
    on_device::Int32
    reserved::Int32
end

mutable struct PredSummary            # svgp_pred_summary (32 bytes): the sums of svgp_predictive / svgp_lik_predictive
    sum_lpd::Float64; sum_sq_err::Float64
    n_points::Int64; n_neg_var::Int64
    PredSummary() = new(0, 0, 0, 0)
end

# ---------------------------------------------------------------------------------------------------------
# context (one per process and GPU) and status -> exception (SURVEY §8b)
# ---------------------------------------------------------------------------------------------------------
const CTX = Ref{Ptr{Cvoid}}(C_NULL)
const AVAILABLE = Ref{Union{Nothing,Bool}}(nothing)

"true when the library can be loaded and sees a GPU (probed once); otherwise every hook declines."
function available()
    if AVAILABLE[] === nothing
        ok = Libdl.dlopen(lib; throw_error=false) !== nothing
        ok = ok && ccall((:svgp_device_count, lib), Int32, ()) > 0
        AVAILABLE[] = ok
    end
    return AVAILABLE[]::Bool
end

function ctx()
    if CTX[] == C_NULL
        dev = parse(Int32, get(ENV, "SVGP_MI355X_DEVICE", "0"))
        st = ccall((:svgp_ctx_create, lib), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), dev, C_NULL, CTX)
        st == 0 || error("svgp_ctx_create failed with status $st")
        # finalizers of DeviceData / DeviceModel run AFTER atexit hooks: the hook clears CTX[] and they skip a dead context
        atexit() do
            c = CTX[]
            CTX[] = C_NULL
            c == C_NULL || ccall((:svgp_ctx_destroy, lib), Int32, (Ptr{Cvoid},), c)
        end
    end
    return CTX[]
end
"free a handle on the live context; after the atexit hook destroyed the context the device memory is gone with it"
free_on_ctx(sym::Symbol, h::Ptr{Cvoid}) = (CTX[] == C_NULL || h == C_NULL) ? Int32(0) :
    (sym === :data ? ccall((:svgp_data_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[], h) :
                     ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[], h))
"""
`worth_offloading(n, M, d; grad=false)`: the library's own small-problem rule (`svgp_offload_advice`, include/svgp_mi355x.h).
A call has a floor of 160-250 us (forward) / ~600 us (value and gradient) whatever the size (profiles/round3/small_problems.md);
the reference's own examples (N = 10 000, M = 20, minibatch 100) sit below the crossover, so every hook declines there and the
pure-Julia method runs.  `ENV["SVGP_OFFLOAD_MIN_WORK"] = "0"` offloads everything.
"""
worth_offloading(n::Integer, M::Integer, d::Integer; grad::Bool=false) =
    ccall((:svgp_offload_advice, lib), Int32, (Int64, Int64, Int32, Int32, Int32), n, M, d, 0, grad ? 1 : 0) == 1

"size of the library communicator on the context (1 without one)"
function comm_world()
    w = Ref{Int32}(1)
    ccall((:svgp_ctx_comm_info, lib), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), ctx(), w, C_NULL)
    return Int(w[])
end
last_error() = unsafe_string(ccall((:svgp_last_error, lib), Cstring, (Ptr{Cvoid},), ctx()))

struct Unsupported <: Exception end   # internal: "decline, the pure-Julia body runs"

function check(st::Integer, terms::Union{Terms,Nothing}=nothing)
    st == 0 && return nothing
    st == 4 && throw(Unsupported())
    st == 1 && throw(ArgumentError(last_error()))
    st == 2 && throw(PosDefException(terms === nothing ? 1 : Int(terms.chol_info)))   # cholesky(Kuu), src/utils.jl:17
    st == 3 && throw(DomainError(-1.0, "sqrt of a negative predictive variance (marginals, SVA:354)"))
    st == 7 && throw(OutOfMemoryError())
    return error("libsvgp_mi355x status $st: " * last_error())
end

# ---------------------------------------------------------------------------------------------------------
# unpacking the reference's objects into the POD description; anything unknown -> Unsupported -> the hook declines
# ---------------------------------------------------------------------------------------------------------
kfamily(::SqExponentialKernel) = Int32(0)
kfamily(::Matern32Kernel) = Int32(1)
kfamily(::Matern52Kernel) = Int32(2)
kfamily(::Any) = nothing

# variance * (Base ∘ ScaleTransform(1/l) | ARDTransform(1 ./ l))  [KernelFunctions: ScaledKernel(kernel, σ²::Vector),
# TransformedKernel(kernel, transform), ScaleTransform(s::Vector), ARDTransform(v::Vector)]
function unpack_kernel(k, d)
    σ² = 1.0
    if k isa ScaledKernel
        σ², k = Float64(only(k.σ²)), k.kernel
    end
    invl = ones(Float64, d)
    if k isa TransformedKernel
        t = k.transform
        if t isa ScaleTransform
            invl = fill(Float64(only(t.s)), d)
        elseif t isa ARDTransform
            length(t.v) == d || return nothing
            invl = collect(Float64, t.v)
        else
            return nothing
        end
        k = k.kernel
    end
    fam = kfamily(k)
    fam === nothing && return nothing
    return fam, σ², invl
end

unpack_mean(::AbstractGPs.ZeroMean) = 0.0
unpack_mean(m::AbstractGPs.ConstMean) = Float64(only(m.c))
unpack_mean(::AbstractGPs.MeanFunction) = 0.0     # any other mean (CustomMean ...): mean_const 0, its values travel as offsets
unpack_mean(::Any) = nothing
# a mean the library takes as caller-evaluated offsets: mux = mean_vector(m, x) at the batch, muz = mean_vector(m, z) at the inducing points
offset_mean(m) = m isa AbstractGPs.MeanFunction && !(m isa AbstractGPs.ZeroMean) && !(m isa AbstractGPs.ConstMean)

# (code, parameter, has a closed-form expectation [GPLikelihoods AnalyticExpectation])
unpack_lik(l::GaussianLikelihood) = (Int32(0), Float64(only(l.σ²)), true)
unpack_lik(::BernoulliLikelihood{<:LogisticLink}) = (Int32(1), 1.0, false)
unpack_lik(::BernoulliLikelihood{<:NormalCDFLink}) = (Int32(5), 1.0, false)   # probit: y ~ Bernoulli(normcdf(f))
unpack_lik(::PoissonLikelihood{<:ExpLink}) = (Int32(2), 1.0, true)
unpack_lik(::ExponentialLikelihood{<:ExpLink}) = (Int32(3), 1.0, true)      # Exponential(scale = exp f), oracle/CONVENTIONS.md
unpack_lik(l::GammaLikelihood{<:Any,<:ExpLink}) = (Int32(4), Float64(only(l.α)), true)   # shape in the parameter slot
unpack_lik(::Any) = nothing

layout(x::ColVecs) = (Int32(0), x.X, size(x.X, 1))
layout(x::RowVecs) = (Int32(1), x.X, size(x.X, 2))
layout(x::AbstractVector{<:Real}) = (Int32(2), x, 1)
layout(::Any) = nothing

# quadrature -> quadrature_n.  AnalyticExpectation on a likelihood WITHOUT a closed form is a MethodError in the reference
# (GPLikelihoods defines no such method): decline, so that the reference body raises exactly that.
function quad_n(q, closed_form::Bool)
    q isa GPLikelihoods.DefaultExpectationMethod && return Int32(0)
    q isa GPLikelihoods.GaussHermiteExpectation && return Int32(length(q.xs))
    q isa GPLikelihoods.AnalyticExpectation && return closed_form ? Int32(0) : nothing
    return nothing
end

isotropic_jitter(Σ::Diagonal{<:Real,<:Fill}) = Float64(Σ[1])          # the types SVA:309 accepts; SVA:314 reads Σy[1]
isotropic_jitter(Σ::ScalMat) = Float64(Σ[1])
isotropic_jitter(::Any) = nothing

"Host arrays a ModelDesc points into; must outlive every ccall that receives the desc (GC.@preserve)."
struct Packed{T}
    invl::Vector{Float64}; Z::Array{T}; m::Vector{T}; Lq::Matrix{T}
    desc::ModelDesc
    ext::Bool        # likelihood not enumerated by the ABI: evaluated HERE on the device marginals (svgp_marginals / svgp_elbo_grad_ext)
    offset::Bool     # an offset mean (offset_mean): desc.mean_const = 0 and the mean's values must travel with every call
end

# Any single-latent GPLikelihoods likelihood can take the host-evaluated route; the two multi-latent ones cannot.
ext_ok(l) = l isa GPLikelihoods.AbstractLikelihood && !(l isa CategoricalLikelihood) && !(l isa HeteroscedasticGaussianLikelihood)

compute_type(::Type{Float32}) = Float32
compute_type(::Type{Float64}) = Float64
compute_type(::Type) = nothing

# offsets = true: the caller passes the offset mean's values with every call (svgp_model_set_mean_z, svgp_*_with_mean) - only the
# hooks below do.  Otherwise a model with an offset mean is refused (Unsupported): the resident / group APIs (DeviceModel, update!,
# elbo_resident, set_model!, elbo(G, ...)) have no offsets, and a zero mean in their place would be a silently wrong ELBO.
function pack(sva::SparseVariationalApproximation{P}, lik, quadrature, ::Type{T}; offsets::Bool=false) where {P,T<:FT}
    lay = layout(sva.fz.x)
    lay === nothing && throw(Unsupported())
    lz, Z, d = lay
    (1 <= d <= 64) || throw(Unsupported())       # SVGP_MAX_D
    sva.fz.f isa AbstractGPs.GP || throw(Unsupported())
    sva.q isa MvNormal || throw(Unsupported())
    ku = unpack_kernel(sva.fz.f.kernel, d)
    c = unpack_mean(sva.fz.f.mean)
    offset = offset_mean(sva.fz.f.mean)
    offset && !offsets && throw(Unsupported())
    lk = unpack_lik(lik)
    ext = lk === nothing
    ext && !ext_ok(lik) && throw(Unsupported())
    ext && (lk = (Int32(0), 1.0, true))        # the descriptor's likelihood slot is unused on the host-evaluated route
    jit = isotropic_jitter(sva.fz.Σy)
    (ku === nothing || c === nothing || jit === nothing) && throw(Unsupported())
    qn = ext ? Int32(0) : quad_n(quadrature, lk[3])
    qn === nothing && throw(Unsupported())
    fam, σ², invl = ku
    m = Vector{T}(mean(sva.q))
    Lq = Matrix{T}(_chol_lower(_chol_cov(sva.q)))          # src/utils.jl:15-18
    Zd = Array{T}(Z)
    desc = ModelDesc(T === Float64 ? 0 : 1, fam, P === Centered ? 1 : 0, lk[1], qn, lz, 0, d, length(m), σ²,
                     pointer(invl), c, jit, lk[2], pointer(Zd), pointer(m), pointer(Lq))
    return Packed{T}(invl, Zd, m, Lq, desc, ext, offset)
end

# ---------------------------------------------------------------------------------------------------------
# elbo(sva, lfx, y; num_data, quadrature)   hook for SVA:340-360   (the FiniteGP method SVA:307-317 and approx_lml
# SVA:276-280 forward to that method unchanged, so they need no hook of their own)
# ---------------------------------------------------------------------------------------------------------
"""
    try_elbo(sva, lfx, y, num_data, quadrature) -> Union{Nothing,Float64}

The ELBO of SVA:340-360 on the device, or `nothing` to let the reference body run.  Called AFTER the prior-identity
check (SVA:347-351), which stays in Julia.  (Method of `MI355XHooks.try_elbo`.)
"""
function MI355XHooks.try_elbo(sva::SparseVariationalApproximation, lfx, y::AbstractVector, num_data, quadrature)
    r = elbo_and_grads(sva, lfx, y, num_data, quadrature, false)
    return r === nothing ? nothing : r[1]
end

# The likelihood-dependent step of SVA:355 kept in Julia: E = expected_loglikelihood(quadrature, lik, marginals, y) on the
# device's marginals and, under AD (`config` = the caller's RuleConfig), its pullback w.r.t. (lik, mu, v).
function host_expectation(config, quadrature, lik, μ::Vector{Float64}, v::Vector{Float64}, y)
    E(l, a, b) = expected_loglikelihood(quadrature, l, Normal.(a, sqrt.(b)), y)      # SVA:354-355
    config === nothing && return sum(E(lik, μ, v)), nothing
    val, back = rrule_via_ad(config, E, lik, μ, v)
    _, Δlik, gμ, gv = back(one(val))
    return val, (Δlik, collect(Float64, unthunk(gμ)), collect(Float64, unthunk(gv)))
end

# value (and, if `want`, the raw gradient blocks) or `nothing`; `config`: the AD rule configuration (host-evaluated route only)
function elbo_and_grads(sva, lfx, y, num_data, quadrature, want::Bool, config=nothing)
    (ENABLED[] && available()) || return nothing
    lay = layout(lfx.fx.x)
    lay === nothing && return nothing
    lx, X, dx = lay
    # the compute type is the inputs' / parameters' float type; the observations only have to convert to it (Bool labels
    # of a Bernoulli likelihood and Int counts of a Poisson one - examples/b-classification/script.jl:58 - are the normal case)
    eltype(y) <: Real || return nothing
    T = compute_type(promote_type(eltype(X), eltype(mean(sva.q))))
    T === nothing && return nothing
    local p
    try
        p = pack(sva, lfx.lik, quadrature, T; offsets=true)
    catch e
        e isa Unsupported || rethrow()
        return nothing
    end
    dx == p.desc.d || return nothing
    # small problems: the Julia body is faster.  NOT under a library communicator: svgp_elbo_host / svgp_elbo_grad are collective
    # there, and a rule decided on this rank's own shard length (or on a rank-local ENV value) would let one rank run the Julia
    # body - and return a shard-local ELBO - while its peers wait in ncclAllReduce (uneven shards, a short last shard).  Every
    # rank of a data-parallel job therefore offloads, whatever its shard's size.
    (comm_world() > 1 || worth_offloading(length(y), length(p.m), Int(p.desc.d); grad=want)) || return nothing
    Xd, yd = Array{T}(X), Vector{T}(y)
    n = length(yd)
    # GP(CustomMean(g), k) and the like: the mean's values at x and z, evaluated here (O(n)); NULL offsets otherwise
    pmean = offset_mean(sva.fz.f.mean)
    μx = pmean ? Vector{T}(AbstractGPs.mean_vector(sva.fz.f.mean, lfx.fx.x)) : T[]
    μz = pmean ? Vector{T}(AbstractGPs.mean_vector(sva.fz.f.mean, sva.fz.x)) : T[]
    pm = Ref(PointMean(pointer(μx), 0, 0))
    gμx = zeros(T, pmean ? n : 0)
    gpm = Ref(PointMeanGrad(pointer(gμx), 0, 0))
    pm_arg = pmean ? pm : Ptr{PointMean}(C_NULL)
    gpm_arg = pmean ? gpm : Ptr{PointMeanGrad}(C_NULL)
    out, terms = Ref{Float64}(), Terms()
    d, M = Int(p.desc.d), length(p.m)
    gl, gz, gm, gLq = zeros(Float64, d), similar(p.Z), similar(p.m), similar(p.Lq)
    g = Grads(0, 0, 0, pointer(gl), pointer(gz), pointer(gm), pointer(gLq))
    gxf = Matrix{T}(undef, n, d)           # d elbo / d x, feature-major (ld = n): RowVecs storage; ColVecs takes its transpose
    gx = InputGrad(pointer(gxf), n, 0, 0)
    st = Int32(0)
    Δlik = nothing
    GC.@preserve p Xd yd gl gz gm gLq gxf μx μz gμx pm gpm begin
        if p.ext
            # host-evaluated likelihood: marginals from the device, SVA:355 here, the backward pass on the device again
            want && config === nothing && return nothing
            # data-parallel contexts: the forward value of this route (svgp_marginals + svgp_prior_kl) is this rank's shard only,
            # while svgp_elbo_grad_ext is collective - value and gradient would disagree; decline (the Julia body runs)
            comm_world() > 1 && return nothing
            hm, hd = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
            μ, v = zeros(Float64, n), zeros(Float64, n)
            try   # the user's likelihood / AD may throw: the handles are freed on every path
            st = ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, hm)
            if st == 0 && pmean
                st = ccall((:svgp_model_set_mean_z, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[], μz)
            end
            if st == 0
                st = ccall((:svgp_data_upload, lib), Int32,
                           (Ptr{Cvoid}, Int32, Int32, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                           ctx(), p.desc.dtype, lx, p.desc.d, n, Xd, C_NULL, hd)
            end
            if st == 0
                st = ccall((:svgp_marginals_with_mean, lib), Int32,
                           (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{Float64}, Ptr{Float64}),
                           ctx(), hm[], hd[], 0, n, pm_arg, μ, v)
            end
            if st == 0
                sumE, pb = host_expectation(want ? config : nothing, quadrature, lfx.lik, μ, v, y)
                if want
                    Δlik, gμ, gv = pb
                    st = ccall((:svgp_elbo_grad_with_mean, lib), Int32,
                               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Ptr{PointMean}, Float64, Ptr{Float64},
                                Ptr{Float64}, Ref{Float64}, Ref{Terms}, Ref{Grads}, Ref{InputGrad}, Ptr{PointMeanGrad}),
                               ctx(), hm[], hd[], 0, n, Float64(num_data), pm_arg, Float64(sumE), gμ, gv, out, terms, g, gx, gpm_arg)
                else
                    kl = Ref{Float64}()
                    st = ccall((:svgp_prior_kl, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}), ctx(), hm[], kl, C_NULL)
                    out[] = sumE * Float64(num_data) / n - kl[]                       # SVA:357-359
                end
            end
            finally
                free_on_ctx(:data, hd[])
                free_on_ctx(:model, hm[])
            end
        elseif !want && !pmean
            # one-shot entry point: uploads x, y, evaluates, frees (resident handles below avoid the upload in loops)
            st = ccall((:svgp_elbo_host, lib), Int32,
                       (Ptr{Cvoid}, Ref{ModelDesc}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ref{Float64}, Ref{Terms}),
                       ctx(), p.desc, lx, n, Xd, yd, Float64(num_data), out, terms)
        else
            hm, hd = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
            st = ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, hm)
            if st == 0 && pmean
                st = ccall((:svgp_model_set_mean_z, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[], μz)
            end
            if st == 0
                st = ccall((:svgp_data_upload, lib), Int32,
                           (Ptr{Cvoid}, Int32, Int32, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                           ctx(), p.desc.dtype, lx, p.desc.d, n, Xd, yd, hd)
            end
            if st == 0 && !want   # (an offset mean's value: resident handles, svgp_elbo_with_mean)
                st = ccall((:svgp_elbo_with_mean, lib), Int32,
                           (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Ptr{PointMean}, Ref{Float64}, Ref{Terms}),
                           ctx(), hm[], hd[], 0, n, Float64(num_data), pm_arg, out, terms)
            elseif st == 0 && pmean
                st = ccall((:svgp_elbo_grad_with_mean, lib), Int32,
                           (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Ptr{PointMean}, Float64, Ptr{Float64},
                            Ptr{Float64}, Ref{Float64}, Ref{Terms}, Ref{Grads}, Ref{InputGrad}, Ptr{PointMeanGrad}),
                           ctx(), hm[], hd[], 0, n, Float64(num_data), pm_arg, 0.0, C_NULL, C_NULL, out, terms, g, gx, gpm_arg)
            elseif st == 0
                st = ccall((:svgp_elbo_grad_inputs, lib), Int32,
                           (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Ref{Float64}, Ref{Terms}, Ref{Grads}, Ref{InputGrad}),
                           ctx(), hm[], hd[], 0, n, Float64(num_data), out, terms, g, gx)
            end
            ccall((:svgp_data_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hd[])
            ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[])
        end
    end
    st == 4 && return nothing            # SVGP_UNSUPPORTED: decline
    check(st, terms)
    # `Δlik`: the likelihood's own tangent from the host pullback (host-evaluated route), to be scaled by num_data / n
    gxl = lx == 0 ? permutedims(gxf) : (lx == 1 ? gxf : vec(gxf))      # in the layout of lfx.fx.x's storage
    # offset mean: mux_bar, and muz_bar = -m_bar (Centered; m enters only through m - muz) or 0 (NonCentered) - include/svgp_mi355x.h
    μz_bar = pmean ? (p.desc.parametrization == 1 ? -Vector{Float64}(gm) : zeros(Float64, M)) : nothing
    return out[], (σ²=g.variance, invl=gl, z=gz, m=gm, Lq=gLq, lik=g.lik_sigma2, c=g.mean_const, x=gxl, Δlik=Δlik, scale=Float64(num_data) / n,
                   μx=pmean ? Vector{Float64}(gμx) : nothing, μz=μz_bar)
end

# ---- structural tangents -------------------------------------------------------------------------------------------
# Mirror images of unpack_kernel / unpack_mean / layout / _chol_cov: each builds the Tangent of exactly the object it unpacked.
function kernel_tangent(k, gσ², ginvl)
    if k isa ScaledKernel
        return Tangent{typeof(k)}(; kernel=inner_kernel_tangent(k.kernel, ginvl), σ²=[oftype(only(k.σ²), gσ²)])
    end
    return inner_kernel_tangent(k, ginvl)
end
function inner_kernel_tangent(k, ginvl)
    k isa TransformedKernel || return NoTangent()           # bare base kernel: no parameters
    t = k.transform
    tt = t isa ScaleTransform ? Tangent{typeof(t)}(; s=[oftype(only(t.s), sum(ginvl))]) :   # invl = fill(s, d)
                                Tangent{typeof(t)}(; v=convert(typeof(t.v), ginvl))
    return Tangent{typeof(k)}(; kernel=NoTangent(), transform=tt)
end
mean_tangent(m::AbstractGPs.ConstMean, gc) = Tangent{typeof(m)}(; c=m.c isa AbstractArray ? [oftype(only(m.c), gc)] : oftype(m.c, gc))
mean_tangent(::Any, gc) = NoTangent()
inputs_tangent(x::Union{ColVecs,RowVecs}, gz) = Tangent{typeof(x)}(; X=convert(typeof(x.X), gz))
inputs_tangent(x::AbstractVector{<:Real}, gz) = convert(typeof(x), vec(gz))

# q = MvNormal(μ, Σ::PDMat): _chol_cov(q) = cholesky(q.Σ) = q.Σ.chol (src/utils.jl:18), so the factor's gradient belongs to
# `Σ.chol.factors` (lower storage: as is; upper storage: transposed); Σ.mat is not read by the NonCentered path.  Other Σ
# types (dense matrix, ScalMat, ...) -> the hook's rrule declines and Zygote differentiates the reference body.
function q_tangent(q::MvNormal, gm, gLq)
    Σ = q.Σ
    Σ isa PDMat || return nothing
    C = Σ.chol
    gf = C.uplo == 'L' ? LowerTriangular(gLq) : UpperTriangular(permutedims(gLq))
    ΔC = Tangent{typeof(C)}(; factors=convert(typeof(C.factors), Matrix(gf)))
    return Tangent{typeof(q)}(; μ=convert(typeof(q.μ), gm), Σ=Tangent{typeof(Σ)}(; chol=ΔC))
end

function lik_tangent(l, glik)
    l isa GaussianLikelihood && return Tangent{typeof(l)}(; σ²=[oftype(only(l.σ²), glik)])
    l isa GammaLikelihood && return Tangent{typeof(l)}(; α=l.α isa AbstractArray ? [oftype(only(l.α), glik)] : oftype(l.α, glik))
    return NoTangent()
end

function ChainRulesCore.rrule(config::RuleConfig{>:HasReverseMode}, ::typeof(MI355XHooks.try_elbo), sva::SparseVariationalApproximation, lfx,
                              y::AbstractVector, num_data, quadrature)
    zero5 = (NoTangent(), NoTangent(), NoTangent(), NoTangent(), NoTangent(), NoTangent())
    decline = (nothing, _ -> zero5)
    sva.q isa MvNormal && sva.q.Σ isa PDMat || return decline       # the tangent of cov(q) is only defined for a stored factor
    r = elbo_and_grads(sva, lfx, y, num_data, quadrature, true, config)
    r === nothing && return decline
    val, g = r
    # an offset mean (CustomMean with learned parameters ...): mux_bar / muz_bar pulled back through mean_vector by the caller's AD
    f0 = sva.fz.f
    mx_back = g.μx === nothing ? nothing : last(rrule_via_ad(config, AbstractGPs.mean_vector, f0.mean, lfx.fx.x))
    mz_back = g.μx === nothing ? nothing : last(rrule_via_ad(config, AbstractGPs.mean_vector, f0.mean, sva.fz.x))
    function try_elbo_pullback(Δ)
        Δ = unthunk(Δ)
        s(a) = Δ .* a
        f = sva.fz.f
        Δmean, Δxm, Δzm = mean_tangent(f.mean, Δ * g.c), NoTangent(), NoTangent()
        if mx_back !== nothing
            _, Δm1, Δxm = mx_back(s(g.μx))
            _, Δm2, Δzm = mz_back(s(g.μz))
            Δmean = unthunk(Δm1) + unthunk(Δm2)
        end
        Δf = Tangent{typeof(f)}(; mean=Δmean, kernel=kernel_tangent(f.kernel, Δ * g.σ², s(g.invl)))
        Δfz = Tangent{typeof(sva.fz)}(; f=Δf, x=inputs_tangent(sva.fz.x, s(g.z)) + unthunk(Δzm))      # Σy (jitter): not differentiated
        Δsva = Tangent{typeof(sva)}(; fz=Δfz, q=q_tangent(sva.q, s(g.m), s(g.Lq)))
        # the prior of lfx is the SAME object (SVA:347-351), its tangent is already on sva.fz.f; the data inputs lfx.fx.x: d elbo / d x
        Δfx = Tangent{typeof(lfx.fx)}(; x=inputs_tangent(lfx.fx.x, s(g.x)) + unthunk(Δxm))
        Δlfx = Tangent{typeof(lfx)}(; fx=Δfx, lik=g.Δlik === nothing ? lik_tangent(lfx.lik, Δ * g.lik) : (Δ * g.scale) * g.Δlik)
        return (NoTangent(), Δsva, Δlfx, NoTangent(), NoTangent(), NoTangent())
    end
    return val, try_elbo_pullback
end

# ---------------------------------------------------------------------------------------------------------
# posterior(sva)   hook for SVA:115-136 (Centered) and SVA:160-187 (NonCentered): the same
# ApproxPosteriorGP(sva, fz.f, (Kuu, B, α)) the reference builds, with the factors computed on the device.
# ---------------------------------------------------------------------------------------------------------
function MI355XHooks.try_posterior(sva::SparseVariationalApproximation{P}) where {P}
    (ENABLED[] && available()) || return nothing
    T = compute_type(eltype(mean(sva.q)))
    T === nothing && return nothing
    local p
    try
        p = pack(sva, GaussianLikelihood(1.0), GPLikelihoods.DefaultExpectationMethod(), T; offsets=true)
    catch e
        e isa Unsupported || rethrow()
        return nothing
    end
    M = length(p.m)
    worth_offloading(0, M, Int(p.desc.d)) || return nothing    # posterior(sva) is M-sized work only: M^3 / 3 against the call's floor
    Lk, α, B = Matrix{T}(undef, M, M), Vector{T}(undef, M), Matrix{T}(undef, M, M)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    st = Int32(0)
    μz = offset_mean(sva.fz.f.mean) ? Vector{T}(AbstractGPs.mean_vector(sva.fz.f.mean, sva.fz.x)) : nothing   # Centered α = Kuu \ (m - mean(fz))
    GC.@preserve p Lk α B μz begin
        st = ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, hm)
        if st == 0 && μz !== nothing
            st = ccall((:svgp_model_set_mean_z, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[], μz)
        end
        if st == 0
            st = ccall((:svgp_posterior, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                       ctx(), hm[], Lk, α, B)
        end
        ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[])
    end
    st == 4 && return nothing
    check(st)        # SVGP_NOT_POSDEF -> PosDefException, as cholesky(Kuu) in the reference (the order is not returned here: 1)
    data = (Kuu=Cholesky(Lk, 'L', 0), B=LowerTriangular(B), α=α)
    return ApproxPosteriorGP(sva, sva.fz.f, data)
end
ChainRulesCore.@non_differentiable available()
# differentiating THROUGH posterior(sva) (nobody in the reference does: elbo has its own rule) uses the Julia body
ChainRulesCore.rrule(::typeof(MI355XHooks.try_posterior), sva::SparseVariationalApproximation) = (nothing, _ -> (NoTangent(), NoTangent()))

# ---------------------------------------------------------------------------------------------------------
# mean / var / cov / mean_and_var / mean_and_cov / cov(x, y)   hooks for SVA:208-264
# ---------------------------------------------------------------------------------------------------------
"`(μ, v, C)` of the approximate posterior at `x` (any of the three may be skipped), or `nothing` to decline."
function MI355XHooks.try_predict(f::ApproxPosteriorGP, x::AbstractVector; want_mean::Bool=true, want_var::Bool=true, want_cov::Bool=false)
    (ENABLED[] && available()) || return nothing
    sva = f.approx
    sva isa SparseVariationalApproximation || return nothing
    lay = layout(x)
    lay === nothing && return nothing
    lx, X, dx = lay
    T = compute_type(eltype(X))
    T === nothing && return nothing
    local p
    try
        p = pack(sva, GaussianLikelihood(1.0), GPLikelihoods.DefaultExpectationMethod(), T; offsets=true)
    catch e
        e isa Unsupported || rethrow()
        return nothing
    end
    dx == p.desc.d || return nothing
    n = length(x)
    worth_offloading(n, length(p.m), Int(p.desc.d)) || return nothing
    Xd = Array{T}(X)
    μ = want_mean ? Vector{T}(undef, n) : nothing
    v = want_var ? Vector{T}(undef, n) : nothing
    C = want_cov ? Matrix{T}(undef, n, n) : nothing
    ptr(a) = a === nothing ? C_NULL : pointer(a)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    st = Int32(0)
    pmean = offset_mean(sva.fz.f.mean)
    μz = pmean ? Vector{T}(AbstractGPs.mean_vector(sva.fz.f.mean, sva.fz.x)) : nothing
    GC.@preserve p Xd μ v C μz begin
        st = ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, hm)
        if st == 0 && pmean
            st = ccall((:svgp_model_set_mean_z, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[], μz)
        end
        if st == 0
            st = ccall((:svgp_predict, lib), Int32,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                       ctx(), hm[], lx, n, Xd, ptr(μ), ptr(v), ptr(C))
        end
        ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[])
    end
    st == 4 && return nothing
    check(st)
    # svgp_predict returns mean_const + K*u α: an offset mean adds its own values at x (SVA:211)
    pmean && μ !== nothing && (μ .+= AbstractGPs.mean_vector(sva.fz.f.mean, x))
    return (μ, v, C)
end

"`cov(f, x, y)` (SVA:255-264) on the device, or `nothing`."
function MI355XHooks.try_cross_cov(f::ApproxPosteriorGP, x::AbstractVector, y::AbstractVector)
    (ENABLED[] && available()) || return nothing
    sva = f.approx
    sva isa SparseVariationalApproximation || return nothing
    lax, lay = layout(x), layout(y)
    (lax === nothing || lay === nothing || lax[1] != lay[1]) && return nothing
    lx, X, dx = lax
    _, Y, dy = lay
    T = compute_type(eltype(X))
    (T === nothing || eltype(Y) !== eltype(X) || dx != dy) && return nothing
    local p
    try
        p = pack(sva, GaussianLikelihood(1.0), GPLikelihoods.DefaultExpectationMethod(), T; offsets=true)   # (cov does not depend on the mean: Lk, B only)
    catch e
        e isa Unsupported || rethrow()
        return nothing
    end
    dx == p.desc.d || return nothing
    nx, ny = length(x), length(y)
    worth_offloading(nx + ny, length(p.m), Int(p.desc.d)) || return nothing
    Xd, Yd = Array{T}(X), Array{T}(Y)
    C = Matrix{T}(undef, nx, ny)
    hm = Ref{Ptr{Cvoid}}(C_NULL)
    st = Int32(0)
    GC.@preserve p Xd Yd C begin
        st = ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, hm)
        if st == 0
            st = ccall((:svgp_predict_cross_cov, lib), Int32,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                       ctx(), hm[], lx, nx, Xd, ny, Yd, C)
        end
        ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), hm[])
    end
    st == 4 && return nothing
    check(st)
    return C
end
# predictions inside a differentiated loss: decline, Zygote differentiates the reference bodies (SVA:208-264)
ChainRulesCore.rrule(::typeof(MI355XHooks.try_predict), f::ApproxPosteriorGP, x::AbstractVector; kw...) = (nothing, _ -> (NoTangent(), NoTangent(), NoTangent()))
ChainRulesCore.rrule(::typeof(MI355XHooks.try_cross_cov), f::ApproxPosteriorGP, x::AbstractVector, y::AbstractVector) = (nothing, _ -> (NoTangent(), NoTangent(), NoTangent(), NoTangent()))

# ---------------------------------------------------------------------------------------------------------
# resident handles for training loops (optional, explicit): upload x, y once, update the model every step
# ---------------------------------------------------------------------------------------------------------
mutable struct DeviceData
    h::Ptr{Cvoid}; n::Int
end
function DeviceData(x, y::AbstractVector{T}) where {T<:FT}
    lx, X, d = layout(x)
    Xd, yd = Array{T}(X), Vector{T}(y)
    h = Ref{Ptr{Cvoid}}()
    GC.@preserve Xd yd check(ccall((:svgp_data_upload, lib), Int32,
        (Ptr{Cvoid}, Int32, Int32, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
        ctx(), T === Float64 ? 0 : 1, lx, d, length(yd), Xd, yd, h))
    D = DeviceData(h[], length(yd))
    finalizer(D -> free_on_ctx(:data, D.h), D)
    return D
end

mutable struct DeviceModel
    h::Ptr{Cvoid}
end
function DeviceModel(p::Packed)
    p.offset && throw(Unsupported())     # (no offsets on the resident path: see pack)
    h = Ref{Ptr{Cvoid}}()
    GC.@preserve p check(ccall((:svgp_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), ctx(), p.desc, h))
    M = DeviceModel(h[])
    finalizer(M -> free_on_ctx(:model, M.h), M)
    return M
end
update!(M::DeviceModel, p::Packed) = p.offset ? throw(Unsupported()) :
    GC.@preserve p check(ccall((:svgp_model_update, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{ModelDesc}), ctx(), M.h, p.desc))

"ELBO of points off+1 : off+len of resident data (a minibatch window), SVA:340-360."
function elbo_resident(M::DeviceModel, D::DeviceData, off::Integer, len::Integer, num_data::Real)
    out, terms = Ref{Float64}(), Terms()
    check(ccall((:svgp_elbo, lib), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Ref{Float64}, Ref{Terms}),
                ctx(), M.h, D.h, off, len, Float64(num_data), out, terms), terms)
    return out[]
end

# ---------------------------------------------------------------------------------------------------------
# multi-GPU from ONE Julia process (svgp_group_*): data sharded over the devices, model replicated, the partial sums of
# SVA:355-359 combined by ONE ncclAllReduce inside the library.  (One process per GPU instead: svgp_comm_unique_id on
# rank 0, the 128 bytes sent with MPI.jl / Distributed.jl, svgp_ctx_attach_comm on every rank; `try_elbo` is then
# collective for the enumerated likelihoods and needs no further change; the host-evaluated-likelihood route declines under a
# communicator - its forward value would be this rank's shard only.)
# ---------------------------------------------------------------------------------------------------------
mutable struct Group
    h::Ptr{Cvoid}; n::Int
    data::Vector{Ptr{Cvoid}}; models::Vector{Ptr{Cvoid}}; shard::Vector{Int64}
end
function Group(devices::Vector{<:Integer})
    h = Ref{Ptr{Cvoid}}()
    ids = Int32.(devices)
    st = ccall((:svgp_group_create, lib), Int32, (Int32, Ptr{Int32}, Ptr{Ptr{Cvoid}}), length(ids), ids, h)
    st == 0 || error("svgp_group_create failed with status $st")
    G = Group(h[], length(ids), Ptr{Cvoid}[], Ptr{Cvoid}[], Int64[])
    finalizer(G) do g
        for i in 1:g.n
            c = ccall((:svgp_group_ctx, lib), Ptr{Cvoid}, (Ptr{Cvoid}, Int32), g.h, i - 1)
            isempty(g.models) || ccall((:svgp_model_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), c, g.models[i])
            isempty(g.data) || ccall((:svgp_data_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), c, g.data[i])
        end
        ccall((:svgp_group_destroy, lib), Int32, (Ptr{Cvoid},), g.h)
    end
    return G
end
group_error(G::Group) = unsafe_string(ccall((:svgp_group_last_error, lib), Cstring, (Ptr{Cvoid},), G.h))
function upload!(G::Group, x, y::AbstractVector{T}) where {T<:FT}
    lx, X, d = layout(x)
    Xd, yd = Array{T}(X), Vector{T}(y)
    G.data = fill(C_NULL, G.n)
    GC.@preserve Xd yd begin
        st = ccall((:svgp_group_data_upload, lib), Int32,
                   (Ptr{Cvoid}, Int32, Int32, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                   G.h, T === Float64 ? 0 : 1, lx, d, length(yd), Xd, yd, G.data)
        st == 0 || error("svgp_group_data_upload: " * group_error(G))
    end
    base, rem = divrem(length(yd), G.n)
    G.shard = [base + (i <= rem ? 1 : 0) for i in 1:G.n]
    return G
end
function set_model!(G::Group, p::Packed)
    p.offset && throw(Unsupported())     # the group calls keep constant means only (include/svgp_mi355x.h)
    GC.@preserve p begin
        if isempty(G.models)
            G.models = fill(C_NULL, G.n)
            st = ccall((:svgp_group_model_create, lib), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Ptr{Cvoid}}), G.h, p.desc, G.models)
        else
            st = ccall((:svgp_group_model_update, lib), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ref{ModelDesc}), G.h, G.models, p.desc)
        end
        st == 0 || error("svgp_group_model_*: " * group_error(G))
    end
    return G
end
"Global ELBO over every member's window `offs[i]+1 : offs[i]+lens[i]` of its shard."
function elbo(G::Group, num_data::Real; offs=zeros(Int64, G.n), lens=G.shard)
    out, terms = Ref{Float64}(), Terms()
    st = ccall((:svgp_group_elbo, lib), Int32,
               (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Float64, Ref{Float64}, Ref{Terms}),
               G.h, G.models, G.data, Int64.(offs), Int64.(lens), Float64(num_data), out, terms)
    st == 0 || (st == 2 ? throw(PosDefException(Int(terms.chol_info))) : error("svgp_group_elbo status $st: " * group_error(G)))
    return out[]
end

# ---------------------------------------------------------------------------------------------------------
# LaplaceApproximation (src/LaplaceApproximationModule.jl): a resident handle over DeviceData (svgp_laplace_*).  Newton mode
# finding, laplace_lml (:157-165), its kernel-parameter gradient and the predictions (:425-463) on the device.  Not hooked into
# the reference's methods (they differentiate through Zygote's rrule of newton_inner_loop); a host calls these directly.
# ---------------------------------------------------------------------------------------------------------
struct LaplaceDesc                    # svgp_laplace_desc (64 bytes)
    dtype::Int32; kernel::Int32; likelihood::Int32; d::Int32; maxiter::Int32; warm_start::Int32
    variance::Float64; inv_lengthscale::Ptr{Float64}; jitter::Float64; lik_sigma2::Float64; reserved::Int64
end
mutable struct LaplaceInfo            # svgp_laplace_info (56 bytes)
    iterations::Int32; converged::Int32; chol_info::Int32; reserved::Int32
    lml::Float64; ms_point::Float64; ms_chol::Float64; ms_linv::Float64; ms_gemv::Float64
    LaplaceInfo() = new(0, 0, 0, 0, 0, 0, 0, 0, 0)
end
mutable struct DeviceLaplace
    h::Ptr{Cvoid}; data::DeviceData
end
function DeviceLaplace(D::DeviceData)
    h = Ref{Ptr{Cvoid}}()
    check(ccall((:svgp_laplace_create, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), ctx(), D.h, h))
    L = DeviceLaplace(h[], D)
    finalizer(L -> (CTX[] == C_NULL || L.h == C_NULL) ||
                   ccall((:svgp_laplace_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[], L.h), L)
    return L
end
"laplace_lml at the Newton mode (desc.warm_start = 1: from the previous call's mode, build_laplace_objective :95-132)."
function laplace_lml!(L::DeviceLaplace, desc::LaplaceDesc; f_init=nothing)
    out, info = Ref{Float64}(), LaplaceInfo()
    GC.@preserve f_init check(ccall((:svgp_laplace_fit, lib), Int32,
                                    (Ptr{Cvoid}, Ptr{Cvoid}, Ref{LaplaceDesc}, Ptr{Cvoid}, Ref{Float64}, Ref{LaplaceInfo}),
                                    ctx(), L.h, desc, f_init === nothing ? C_NULL : pointer(f_init), out, info))
    return out[], info
end
"laplace_lml and its gradient with respect to (variance, inv_lengthscale): what Zygote gets from the rrule of :330-369."
function laplace_lml_and_grad!(L::DeviceLaplace, desc::LaplaceDesc; f_init=nothing)
    out, info, gv = Ref{Float64}(), LaplaceInfo(), Ref{Float64}()
    gl = zeros(Float64, desc.d)
    GC.@preserve f_init gl check(ccall((:svgp_laplace_lml_grad, lib), Int32,
                                       (Ptr{Cvoid}, Ptr{Cvoid}, Ref{LaplaceDesc}, Ptr{Cvoid}, Ref{Float64}, Ref{LaplaceInfo}, Ref{Float64},
                                        Ptr{Float64}),
                                       ctx(), L.h, desc, f_init === nothing ? C_NULL : pointer(f_init), out, info, gv, gl))
    return out[], gv[], gl, info
end
"(f_opt, d_loglik, W) of the cached intermediates (LaplaceCache :180-199)."
function laplace_mode(L::DeviceLaplace, ::Type{T}) where {T<:FT}
    f, g, w = zeros(T, L.data.n), zeros(T, L.data.n), zeros(T, L.data.n)
    check(ccall((:svgp_laplace_mode, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), L.h, f, g, w))
    return f, g, w
end
npoints(lx, X) = lx == 1 ? size(X, 1) : (lx == 0 ? size(X, 2) : length(X))
"mean_and_var / mean_and_cov of the LaplacePosteriorGP at x (:437-447)."
function laplace_predict(L::DeviceLaplace, x, ::Type{T}; want_cov::Bool=false) where {T<:FT}
    lx, X, _ = layout(x)
    Xd = Array{T}(X)
    n = npoints(lx, Xd)
    μ, v = zeros(T, n), zeros(T, n)
    C = want_cov ? zeros(T, n, n) : nothing
    GC.@preserve Xd check(ccall((:svgp_laplace_predict, lib), Int32,
                                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                ctx(), L.h, lx, n, Xd, μ, v, C === nothing ? C_NULL : C))
    return μ, v, C
end
"cov(f, x, y) of the LaplacePosteriorGP (:458-463)."
function laplace_cross_cov(L::DeviceLaplace, x, y, ::Type{T}) where {T<:FT}
    lx, X, _ = layout(x)
    _, Y, _ = layout(y)
    Xd, Yd = Array{T}(X), Array{T}(Y)
    nx, ny = npoints(lx, Xd), npoints(lx, Yd)
    C = zeros(T, nx, ny)
    GC.@preserve Xd Yd check(ccall((:svgp_laplace_predict_cross_cov, lib), Int32,
                                   (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                                   ctx(), L.h, lx, nx, Xd, ny, Yd, C))
    return C
end

# ---------------------------------------------------------------------------------------------------------
# NearestNeighbors(k) (src/NearestNeighborsModule.jl): a resident handle over DeviceData (svgp_nn_*).  approx_lml (:108-113), its
# gradient with respect to (variance, inv_lengthscale, diag), posterior (:97-106) and the predictions on the device.  The
# neighbours of a point are the k points before it in the order of D.  Not hooked into the reference's methods; a host calls these.
# ---------------------------------------------------------------------------------------------------------
struct NNDesc                         # svgp_nn_desc (56 bytes)
    dtype::Int32; kernel::Int32; d::Int32; k::Int32
    variance::Float64; inv_lengthscale::Ptr{Float64}; diag::Float64; mean_const::Float64; reserved::Int64
end
mutable struct NNInfo                 # svgp_nn_info (24 bytes)
    first_bad::Int64; n_neg_f::Int64; lml::Float64
    NNInfo() = new(0, 0, 0)
end
mutable struct DeviceNN
    h::Ptr{Cvoid}; data::DeviceData
end
function DeviceNN(D::DeviceData)
    h = Ref{Ptr{Cvoid}}()
    check(ccall((:svgp_nn_create, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), ctx(), D.h, h))
    N = DeviceNN(h[], D)
    finalizer(N -> (CTX[] == C_NULL || N.h == C_NULL) ||
                   ccall((:svgp_nn_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[], N.h), N)
    return N
end
nn_check(st, info::NNInfo) = st == 2 ? throw(PosDefException(Int(info.first_bad))) : check(st)
"Condition point i on row i of `table` (n × kb Int32, 0-based indices of earlier points, the valid ones first, -1 after them)."
function nn_set_neighbors!(N::DeviceNN, k::Integer, table::Matrix{Int32})
    GC.@preserve table check(ccall((:svgp_nn_set_neighbors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}),
                                   ctx(), N.h, Int32(k), table))
    return N
end
"The exact k nearest predecessors of every point under the metric `inv_lengthscale` (nothing: ones), built on the device."
function nn_build_neighbors!(N::DeviceNN, k::Integer, inv_lengthscale::Union{Nothing,Vector{Float64}}=nothing)
    il = inv_lengthscale === nothing ? Ptr{Float64}(C_NULL) : pointer(inv_lengthscale)
    GC.@preserve inv_lengthscale check(ccall((:svgp_nn_build_neighbors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}),
                                             ctx(), N.h, Int32(k), il))
    return N
end
"The handle's neighbour table (n × kb Int32), or nothing when the window of the previous k points is in use."
function nn_neighbors(N::DeviceNN)
    kb = Ref{Int32}(-1)
    check(ccall((:svgp_nn_get_neighbors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), ctx(), N.h, kb, C_NULL))
    kb[] < 0 && return nothing
    table = zeros(Int32, N.data.n, kb[])
    check(ccall((:svgp_nn_get_neighbors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), ctx(), N.h, kb, table))
    return table
end
"Back to the window of the previous k points."
nn_clear_neighbors!(N::DeviceNN) = (check(ccall((:svgp_nn_clear_neighbors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), N.h)); N)
"approx_lml(NearestNeighbors(desc.k), fx, y) (:108-113); desc.diag = 0 is the reference, which ignores fx.Σy."
function nn_lml!(N::DeviceNN, desc::NNDesc)
    out, info = Ref{Float64}(), NNInfo()
    nn_check(ccall((:svgp_nn_lml, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{NNDesc}, Ref{Float64}, Ref{NNInfo}),
                   ctx(), N.h, desc, out, info), info)
    return out[], info
end
"approx_lml and its gradient with respect to (variance, inv_lengthscale, diag)."
function nn_lml_and_grad!(N::DeviceNN, desc::NNDesc)
    out, info, gv, gd = Ref{Float64}(), NNInfo(), Ref{Float64}(), Ref{Float64}()
    gl = zeros(Float64, desc.d)
    GC.@preserve gl nn_check(ccall((:svgp_nn_lml_grad, lib), Int32,
                                   (Ptr{Cvoid}, Ptr{Cvoid}, Ref{NNDesc}, Ref{Float64}, Ref{NNInfo}, Ref{Float64}, Ptr{Float64}, Ref{Float64}),
                                   ctx(), N.h, desc, out, info, gv, gl, gd), info)
    return out[], gv[], gl, gd[], info
end
"posterior(NearestNeighbors(desc.k), fx, y) (:97-106): caches B, F and α on the device; returns approx_lml."
function nn_fit!(N::DeviceNN, desc::NNDesc)
    out, info = Ref{Float64}(), NNInfo()
    nn_check(ccall((:svgp_nn_fit, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{NNDesc}, Ref{Float64}, Ref{NNInfo}),
                   ctx(), N.h, desc, out, info), info)
    return out[], info
end
"(B banded n × kb, F, α) of the last nn_fit!, kb = min(k, n - 1): B[i, t] is the coefficient of point i on point i - kb + t, or with a
neighbour table on point table[i, t]."
function nn_factors(N::DeviceNN, k::Integer, ::Type{T}) where {T<:FT}
    n = N.data.n
    B, F, α = zeros(T, n, min(k, n - 1)), zeros(T, n), zeros(T, n)
    check(ccall((:svgp_nn_factors, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx(), N.h, B, F, α))
    return B, F, α
end
"mean_and_var / mean_and_cov of the PosteriorGP with C = InvRoot(U) at x."
function nn_predict(N::DeviceNN, x, ::Type{T}; want_cov::Bool=false) where {T<:FT}
    lx, X, _ = layout(x)
    Xd = Array{T}(X)
    n = npoints(lx, Xd)
    μ, v = zeros(T, n), zeros(T, n)
    C = want_cov ? zeros(T, n, n) : nothing
    GC.@preserve Xd check(ccall((:svgp_nn_predict, lib), Int32,
                                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                ctx(), N.h, lx, n, Xd, μ, v, C === nothing ? C_NULL : C))
    return μ, v, C
end
"Nearest-neighbour kriging at x: every test point conditioned on its min(k, n) nearest training points under the fit's inverse
lengthscales (no N × n* object).  -> (μ, v, table), table n* × min(k, n) zero-based indices (-1 after a short row) when want_table."
function predict_local(N::DeviceNN, x, k::Integer, ::Type{T}; want_table::Bool=false) where {T<:FT}
    lx, X, _ = layout(x)
    Xd = Array{T}(X)
    n = npoints(lx, Xd)
    μ, v = zeros(T, n), zeros(T, n)
    table = want_table ? zeros(Int32, n, min(k, N.data.n)) : nothing
    GC.@preserve Xd check(ccall((:svgp_nn_predict_local, lib), Int32,
                                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}),
                                ctx(), N.h, lx, n, Xd, k, μ, v, table === nothing ? C_NULL : table))
    return μ, v, table
end
"cov(f, x, y) of the same posterior."
function nn_cross_cov(N::DeviceNN, x, y, ::Type{T}) where {T<:FT}
    lx, X, _ = layout(x)
    _, Y, _ = layout(y)
    Xd, Yd = Array{T}(X), Array{T}(Y)
    nx, ny = npoints(lx, Xd), npoints(lx, Yd)
    C = zeros(T, nx, ny)
    GC.@preserve Xd Yd check(ccall((:svgp_nn_predict_cross_cov, lib), Int32,
                                   (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                                   ctx(), N.h, lx, nx, Xd, ny, Yd, C))
    return C
end

# ---------------------------------------------------------------------------------------------------------
# The collapsed (Titsias 2009, eqs. 11 / 12) bound and the optimal q(u) on resident handles (svgp_collapsed_*): what the reference's
# tests build on the host with optimal_variational_posterior (test/test_utils.jl:7-17) and compare with posterior(VFE(fz), fx, y)
# (test/SparseVariationalApproximationModule.jl:99-134).  Gaussian likelihood, ZeroMean / ConstMean, one GPU.  Not hooked into the
# reference's methods; a host calls these.
# ---------------------------------------------------------------------------------------------------------
mutable struct CollapsedTerms         # svgp_collapsed_terms (64 bytes)
    bound::Float64; fit::Float64; trace::Float64; logdet_B::Float64; logdet_kuu::Float64
    n_points::Int64; chol_info::Int32; chol_info_b::Int32; reserved::Int64
    CollapsedTerms() = new(0, 0, 0, 0, 0, 0, 0, 0, 0)
end
collapsed_check(st, t::CollapsedTerms) =
    st == 2 ? throw(PosDefException(Int(t.chol_info != 0 ? t.chol_info : t.chol_info_b))) : check(st)
"The collapsed bound over the points off+1 : off+len of D (the model's q is neither read nor changed)."
function collapsed_bound(Mo::DeviceModel, D::DeviceData; off::Integer=0, len::Integer=D.n - off)
    out, t = Ref{Float64}(), CollapsedTerms()
    collapsed_check(ccall((:svgp_collapsed_bound, lib), Int32,
                          (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{Float64}, Ref{CollapsedTerms}),
                          ctx(), Mo.h, D.h, off, len, out, t), t)
    return out[], t
end
"Writes the optimal q into the model's device-resident m / Lq (its own parametrisation); returns (bound, m, Lq) as host arrays."
function collapsed_q!(Mo::DeviceModel, D::DeviceData, M::Integer, ::Type{T}; off::Integer=0, len::Integer=D.n - off) where {T<:FT}
    out = Ref{Float64}()
    m, Lq = zeros(T, M), zeros(T, M, M)
    check(ccall((:svgp_collapsed_q, lib), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
                ctx(), Mo.h, D.h, off, len, m, Lq, out))
    return out[], m, LowerTriangular(Lq)
end
"The bound and its total derivatives in (variance, lik_sigma2, mean_const, inv_lengthscale, z); z_bar is d × M (ColVecs storage)."
function collapsed_bound_and_grad!(Mo::DeviceModel, D::DeviceData, M::Integer, d::Integer, ::Type{T};
                                   off::Integer=0, len::Integer=D.n - off) where {T<:FT}
    out, t = Ref{Float64}(), CollapsedTerms()
    gl, gz = zeros(Float64, d), zeros(T, d, M)
    g = Grads(0.0, 0.0, 0.0, pointer(gl), pointer(gz), C_NULL, C_NULL)
    GC.@preserve gl gz collapsed_check(ccall((:svgp_collapsed_grad, lib), Int32,
                                             (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{Float64}, Ref{CollapsedTerms}, Ref{Grads}, Ptr{Cvoid}),
                                             ctx(), Mo.h, D.h, off, len, out, t, g, C_NULL), t)
    return out[], t, (variance=g.variance, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const, inv_lengthscale=gl, z=gz)
end

# ... with per-point noise variances Σy = Diagonal(lik_sigma2 .+ s) and prior mean offsets mux (svgp_collapsed_*_with_noise): what
# AbstractGPs' VFE computes for f(x, Σy::Diagonal) and any mean function.  s, mux: host vectors of the data's element type, one entry
# per point of the window, or `nothing`; a model carrying muz (svgp_model_set_mean_z) is accepted.
point_noise_arg(s::Nothing) = Ptr{PointNoise}(C_NULL)
point_noise_arg(s::Vector) = Ref(PointNoise(pointer(s), 0, 0))
point_mean_arg(mux::Nothing) = Ptr{PointMean}(C_NULL)
point_mean_arg(mux::Vector) = Ref(PointMean(pointer(mux), 0, 0))
"The collapsed bound over the points off+1 : off+len of D with noise variances lik_sigma2 .+ s and prior mean mean_const .+ mux."
function collapsed_bound_with_noise(Mo::DeviceModel, D::DeviceData; s=nothing, mux=nothing, off::Integer=0, len::Integer=D.n - off)
    out, t = Ref{Float64}(), CollapsedTerms()
    pm, pn = point_mean_arg(mux), point_noise_arg(s)
    GC.@preserve s mux collapsed_check(ccall((:svgp_collapsed_bound_with_noise, lib), Int32,
                                             (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{PointNoise}, Ref{Float64}, Ref{CollapsedTerms}),
                                             ctx(), Mo.h, D.h, off, len, pm, pn, out, t), t)
    return out[], t
end
"Writes that problem's optimal q into the model's device-resident m / Lq; returns (bound, m, Lq) as host arrays."
function collapsed_q_with_noise!(Mo::DeviceModel, D::DeviceData, M::Integer, ::Type{T}; s=nothing, mux=nothing, off::Integer=0,
                                 len::Integer=D.n - off) where {T<:FT}
    out = Ref{Float64}()
    m, Lq = zeros(T, M), zeros(T, M, M)
    pm, pn = point_mean_arg(mux), point_noise_arg(s)
    GC.@preserve s mux check(ccall((:svgp_collapsed_q_with_noise, lib), Int32,
                                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{PointNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
                                   ctx(), Mo.h, D.h, off, len, pm, pn, m, Lq, out))
    return out[], m, LowerTriangular(Lq)
end
"The bound and its total derivatives, with s_bar = d bound / d Σy_jj and mux_bar = d bound / d mean(x_j) (host vectors of length len)."
function collapsed_bound_and_grad_with_noise!(Mo::DeviceModel, D::DeviceData, M::Integer, d::Integer, ::Type{T}; s=nothing, mux=nothing,
                                              off::Integer=0, len::Integer=D.n - off) where {T<:FT}
    out, t = Ref{Float64}(), CollapsedTerms()
    gl, gz = zeros(Float64, d), zeros(T, d, M)
    sbar, mbar = zeros(T, len), zeros(T, len)
    g = Grads(0.0, 0.0, 0.0, pointer(gl), pointer(gz), C_NULL, C_NULL)
    pm, pn = point_mean_arg(mux), point_noise_arg(s)
    gpm, gpn = Ref(PointMeanGrad(pointer(mbar), 0, 0)), Ref(PointNoiseGrad(pointer(sbar), 0, 0))
    GC.@preserve gl gz s mux sbar mbar collapsed_check(ccall((:svgp_collapsed_grad_with_noise, lib), Int32,
                                                             (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{PointNoise}, Ref{Float64}, Ref{CollapsedTerms}, Ref{Grads}, Ptr{Cvoid}, Ptr{PointMeanGrad}, Ptr{PointNoiseGrad}),
                                                             ctx(), Mo.h, D.h, off, len, pm, pn, out, t, g, C_NULL, gpm, gpn), t)
    return out[], t, (variance=g.variance, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const, inv_lengthscale=gl, z=gz, s=sbar, mux=mbar)
end

# ---------------------------------------------------------------------------------------------------------
# Natural-gradient steps on q(u) on resident handles (svgp_natgrad_step / svgp_model_update_keep_q): q moves on the device along the
# ELBO's gradient in the expectation parameters (the ELBO of SVA:340-373), the host's optimiser keeps the hyperparameters and z.  Any
# built-in likelihood, any minibatch window with num_data, step length gamma in (0, 1]; one GPU, ZeroMean / ConstMean.
# ---------------------------------------------------------------------------------------------------------
"One natural-gradient step of length `gamma` on the model's device-resident q over the points off+1 : off+len of D.  Returns
(elbo, grads, m, Lq): the ELBO and its gradient in (variance, lik_sigma2, mean_const, inv_lengthscale, z) at the q the call STARTED
from (what svgp_elbo_grad returns), and the NEW q as host arrays in the model's parametrisation."
function natgrad_step!(Mo::DeviceModel, D::DeviceData, M::Integer, d::Integer, ::Type{T}; gamma::Real=1.0, num_data::Real=0.0,
                       off::Integer=0, len::Integer=D.n - off) where {T<:FT}
    out, terms = Ref{Float64}(), Terms()
    gl, gz = zeros(Float64, d), zeros(T, d, M)
    m, Lq = zeros(T, M), zeros(T, M, M)
    g = Grads(0.0, 0.0, 0.0, pointer(gl), pointer(gz), C_NULL, C_NULL)
    GC.@preserve gl gz check(ccall((:svgp_natgrad_step, lib), Int32,
                                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Float64, Ref{Float64}, Ref{Terms}, Ref{Grads}, Ptr{Cvoid}, Ptr{Cvoid}),
                                   ctx(), Mo.h, D.h, off, len, Float64(num_data), Float64(gamma), out, terms, g, m, Lq), terms)
    return out[], (variance=g.variance, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const, inv_lengthscale=gl, z=gz), m, LowerTriangular(Lq)
end
"The same step with the caller's point gradients (sum_e, g_mu, g_v as for svgp_elbo_grad_ext); returns (elbo, m, Lq)."
function natgrad_step_ext!(Mo::DeviceModel, D::DeviceData, M::Integer, ::Type{T}, sum_e::Real, g_mu::Vector{Float64}, g_v::Vector{Float64};
                           gamma::Real=1.0, num_data::Real=0.0, off::Integer=0, len::Integer=D.n - off) where {T<:FT}
    (length(g_mu) == len && length(g_v) == len) || throw(ArgumentError("one point gradient per point of the batch"))
    out, terms = Ref{Float64}(), Terms()
    m, Lq = zeros(T, M), zeros(T, M, M)
    check(ccall((:svgp_natgrad_step_ext, lib), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Terms}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), Mo.h, D.h, off, len, Float64(num_data), Float64(gamma), Float64(sum_e), g_mu, g_v, out, terms, C_NULL, m, Lq), terms)
    return out[], m, LowerTriangular(Lq)
end
"update! without the upload of q: the packed m / Lq are ignored, the device-resident q (e.g. what natgrad_step! wrote) stays."
update_keep_q!(M::DeviceModel, p::Packed) = p.offset ? throw(Unsupported()) :
    GC.@preserve p check(ccall((:svgp_model_update_keep_q, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{ModelDesc}), ctx(), M.h, p.desc))

# ---------------------------------------------------------------------------------------------------------
# The predictive distribution of the OBSERVATION (svgp_predictive / svgp_lik_predictive): log p(y_i | D) = log ∫ p(y_i | f) N(f; μ_i, v_i) df
# and (E[y_i], Var[y_i]) through the model's likelihood - what AbstractGPs / GPLikelihoods leave to the caller after marginals(f_post(x)).
# NLPD = -mean(lpd); RMSE = sqrt(summary.sum_sq_err / summary.n_points).  Always local: a data-parallel host adds the ranks' summaries.
# ---------------------------------------------------------------------------------------------------------
"Held-out metrics and predictions of y for the points off+1 : off+len of resident data: one forward data pass, then the likelihood on
the device.  Returns (summary, lpd, ymean, yvar); `mux`: the batch's prior mean offsets (data eltype) or nothing.  Data without y:
call with `with_y=false` and read ymean / yvar only."
function predictive(Mo::DeviceModel, D::DeviceData; off::Integer=0, len::Integer=D.n - off, mux::Union{Nothing,Vector}=nothing,
                    with_y::Bool=true)
    s = PredSummary()
    lpd, ymean, yvar = zeros(Float64, with_y ? len : 0), zeros(Float64, len), zeros(Float64, len)
    mux === nothing || length(mux) == len || throw(ArgumentError("one prior mean offset per point of the batch"))
    pm = mux === nothing ? Ref(PointMean(C_NULL, 0, 0)) : Ref(PointMean(pointer(mux), 0, 0))
    GC.@preserve mux pm check(ccall((:svgp_predictive, lib), Int32,
                                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{PredSummary}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                    ctx(), Mo.h, D.h, off, len,
                                    mux === nothing ? Ptr{PointMean}(C_NULL) : Base.unsafe_convert(Ptr{PointMean}, pm),
                                    with_y ? Ptr{PredSummary}(pointer_from_objref(s)) : Ptr{PredSummary}(C_NULL),
                                    with_y ? pointer(lpd) : Ptr{Float64}(C_NULL), ymean, yvar))
    return s, lpd, ymean, yvar
end
"The same point stage on latent marginals the caller holds (Laplace, NearestNeighbors, svgp_marginals' output): no model, no data pass.
`lik` is a SVGP_LIK_* code, `param` the Gaussian σ² / the Gamma shape; `y === nothing`: the moments alone.  Returns (summary, lpd, ymean, yvar)."
function lik_predictive(lik::Integer, param::Real, mu::Vector{Float64}, var::Vector{Float64}, y::Union{Nothing,Vector{Float64}}=nothing;
                        quadrature_n::Integer=0)
    n = length(mu)
    (length(var) == n && (y === nothing || length(y) == n)) || throw(ArgumentError("mu, var and y must have one entry per point"))
    s = PredSummary()
    lpd, ymean, yvar = zeros(Float64, y === nothing ? 0 : n), zeros(Float64, n), zeros(Float64, n)
    GC.@preserve y check(ccall((:svgp_lik_predictive, lib), Int32,
                               (Ptr{Cvoid}, Int32, Float64, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{PredSummary}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                               ctx(), Int32(lik), Float64(param), Int32(quadrature_n), n, mu, var,
                               y === nothing ? Ptr{Float64}(C_NULL) : pointer(y),
                               y === nothing ? Ptr{PredSummary}(C_NULL) : Ptr{PredSummary}(pointer_from_objref(s)),
                               y === nothing ? Ptr{Float64}(C_NULL) : pointer(lpd), ymean, yvar))
    return s, lpd, ymean, yvar
end

# ---------------------------------------------------------------------------------------------------------
# Pathwise posterior function samples (svgp_sampler_*): `rand(f_post(x), S)` as S FUNCTIONS resident on the device, evaluated at any
# points, any number of times, in one data pass linear in the number of points - f = mean + Φ w + k(·, z) V with V from u ~ q(u)
# (Wilson et al. 2020).  The library draws nothing: Ω (unit-lengthscale frequencies, d × L), τ (L), W (L × S), E (M × S) are the
# caller's (SE: Ω ~ N(0, I); Matern-ν: g sqrt(2ν / χ²_{2ν})).  The Fourier part approximates the prior with error O(σ² / sqrt(L)); the
# update term is exact.
# ---------------------------------------------------------------------------------------------------------
struct SampleBasis                    # svgp_sample_basis (48 bytes)
    n_features::Int64
    n_samples::Int64
    omega::Ptr{Cvoid}
    tau::Ptr{Cvoid}
    w::Ptr{Cvoid}
    eps::Ptr{Cvoid}
end

mutable struct DeviceSampler
    h::Ptr{Cvoid}; S::Int; M::Int
end
"A snapshot of S function samples of the model's posterior.  Ω is d × L, τ has L entries, W is L × S, E is M × S (Julia's column-major
storage of these is the C-ABI's [L][d], [S][L] and [S][M]); all in the model's element type."
function DeviceSampler(Mo::DeviceModel, Ω::Matrix{T}, τ::Vector{T}, W::Matrix{T}, E::Matrix{T}) where {T<:FT}
    L, S, M = length(τ), size(E, 2), size(E, 1)
    (size(Ω, 2) == L && size(W) == (L, S)) || throw(ArgumentError("Ω must be d × L, τ of length L, W L × S, E M × S"))
    h = Ref{Ptr{Cvoid}}()
    b = SampleBasis(L, S, L > 0 ? pointer(Ω) : C_NULL, L > 0 ? pointer(τ) : C_NULL, L > 0 ? pointer(W) : C_NULL, pointer(E))
    GC.@preserve Ω τ W E check(ccall((:svgp_sampler_create, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SampleBasis}, Ptr{Ptr{Cvoid}}),
                                     ctx(), Mo.h, b, h))
    Sm = DeviceSampler(h[], S, M)
    finalizer(s -> (CTX[] == C_NULL || s.h == C_NULL) ||
                   ccall((:svgp_sampler_free, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[], s.h), Sm)
    return Sm
end
"The S functions at the points off+1 : off+len of resident data: a len × S matrix (column s = f_s), in the data's element type `T`.
`mux`: the window's prior mean offsets or nothing."
function sample_functions(Sm::DeviceSampler, D::DeviceData, ::Type{T}; off::Integer=0, len::Integer=D.n - off,
                          mux::Union{Nothing,Vector}=nothing) where {T<:FT}
    mux === nothing || length(mux) == len || throw(ArgumentError("one prior mean offset per point of the window"))
    out = zeros(T, len, Sm.S)
    pm = mux === nothing ? Ref(PointMean(C_NULL, 0, 0)) : Ref(PointMean(pointer(mux), 0, 0))
    GC.@preserve mux pm check(ccall((:svgp_sampler_eval, lib), Int32,
                                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{Cvoid}, Int64, Int32),
                                    ctx(), Sm.h, D.h, off, len,
                                    mux === nothing ? Ptr{PointMean}(C_NULL) : Base.unsafe_convert(Ptr{PointMean}, pm),
                                    out, len, Int32(0)))
    return out
end
"The S functions and their input gradients at the points off+1 : off+len of resident data: `(F, G)` with F len × S (as
`sample_functions`, bitwise; `nothing` with `values=false`) and G len × d × S, `G[j, c, s] = ∂f_s/∂x_c` at point j.  G is the gradient of
f_s minus the prior mean: the Jacobian of the caller's own offsets `mux` is the caller's to add."
function sample_gradients(Sm::DeviceSampler, D::DeviceData, ::Type{T}, d::Integer; off::Integer=0, len::Integer=D.n - off,
                          mux::Union{Nothing,Vector}=nothing, values::Bool=true) where {T<:FT}
    mux === nothing || length(mux) == len || throw(ArgumentError("one prior mean offset per point of the window"))
    F = zeros(T, len, values ? Sm.S : 0)
    G = zeros(T, len, d, Sm.S)       # d: the input dimension of the data and the sampler
    pm = mux === nothing ? Ref(PointMean(C_NULL, 0, 0)) : Ref(PointMean(pointer(mux), 0, 0))
    GC.@preserve mux pm F G check(ccall((:svgp_sampler_eval_grad, lib), Int32,
                                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{PointMean}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32),
                                        ctx(), Sm.h, D.h, off, len,
                                        mux === nothing ? Ptr{PointMean}(C_NULL) : Base.unsafe_convert(Ptr{PointMean}, pm),
                                        values ? Ptr{Cvoid}(pointer(F)) : C_NULL, len, G, len, Int32(0)))
    return (values ? F : nothing), G
end
"(u, V) of the sampler in Float64, M × S each: the draws u_s ~ q(u) and V_s = Kuu \\ (u_s - mean(z) - Φ(z) w_s)."
function sampler_state(Sm::DeviceSampler)
    u, V = zeros(Float64, Sm.M, Sm.S), zeros(Float64, Sm.M, Sm.S)
    check(ccall((:svgp_sampler_state, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx(), Sm.h, u, V))
    return u, V
end

end # module
