# CFMMRouterAMD.jl -- the Julia host side of the MI355X drop-in: a `Router`-compatible type whose
# `find_arb!` sweep and Ψ/dual reductions run in libcfmm_amd.so (include/cfmm_amd.h) while
# LBFGSB.jl keeps driving the outer loop exactly as in CFMMRouter.jl's src/router.jl:58-108.
#
# STATUS: EXPERIMENTAL -- written against Julia 1.7+/CFMMRouter v0.3.1 but NEVER EXECUTED: there is no
# Julia toolchain in the build image.  Every ccall below has a twin that IS executed on the MI355X:
# the plain-C clients tests/c/abi_smoke.c and tests/c/abi_multi.c (same entry points, same argument
# order) and the Python mirror (cfmmrouter.jl_amd/router.py, tests/test_gpu_*.py).  The one-command check for whoever has
# Julia and an MI355X:   CFMM_AMD_LIB=$PWD/cfmmrouter.jl_amd/libcfmm_amd.so julia --project=julia -e 'using Pkg; Pkg.test()'
# (julia/test/runtests.jl: the reference's own router / CFMM tests through AMDRouter).
#
# Usage (drop-in for the README quick start):
#     using CFMMRouter, CFMMRouterAMD
#     router = AMDRouter(LinearNonnegative(prices), [equal_pool, unequal_small_pool], 2)
#     route!(router); Ψ = netflows(router)
module CFMMRouterAMD

using CFMMRouter
using CFMMRouter: CFMM, ProductTwoCoin, GeometricMeanTwoCoin, UniV3, Objective, Product, GeometricMean, Curve
using LBFGSB
import CFMMRouter: route!, netflows, netflows!, find_arb!, update_reserves!, forward_trade

export AMDRouter, route_native!, polish!, update_pools!, swap!, select_trades, quote_swaps, quote_swaps_out, quote_paths, quote_paths_out, swap_paths!, swap_out!, swap_paths_out!, find_paths, find_paths_out, size_paths, split_paths, find_disjoint_paths, split_paths_out, find_disjoint_paths_out, swap_orders!, swap_orders_out!, quote_rate, spot_price, quote_path_rate, amount_to_rate, swap_limit!, forward_trade, backward_trade, SolidlyStableTwoCoin

const LIB = get(ENV, "CFMM_AMD_LIB", "libcfmm_amd.so")

# The "stable" pair of the Solidly family (Velodrome, Aerodrome and forks): φ(R) = R₁³R₂ + R₁R₂³ on decimal-normalised
# balances.  CFMMRouter.jl has no such pool; this type exists for the device, which solves its arbitrage problem in
# closed form (include/cfmm_amd.h, cfmm_pools_add_solidly).  Fields and constructor arguments of ProductTwoCoin
# (src/cfmms.jl:101-111); 0 < γ <= 1 and reserves within [2^-150, 2^150] are checked at upload.
struct SolidlyStableTwoCoin{T} <: CFMM{T}
    R::Vector{T}
    γ::T
    Ai::Vector{UInt}
    function SolidlyStableTwoCoin(R, γ, idx)
        length(R) == 2 || throw(ArgumentError("length of R must be 2 for *TwoCoin constructors"))
        length(idx) == 2 || throw(ArgumentError("length of idx must be 2 for *TwoCoin constructors"))
        T = eltype(float.(R))
        return new{T}(collect(T, R), convert(T, γ), convert.(UInt, collect(idx)))
    end
end
CFMMRouter.ϕ(c::SolidlyStableTwoCoin; R=nothing) = (R = isnothing(R) ? c.R : R; R[1] * R[2] * (R[1]^2 + R[2]^2))
function CFMMRouter.∇ϕ!(x, c::SolidlyStableTwoCoin; R=nothing)
    R = isnothing(R) ? c.R : R
    x[1] = R[2] * (3 * R[1]^2 + R[2]^2)
    x[2] = R[1] * (R[1]^2 + 3 * R[2]^2)
    return nothing
end

struct CFMMAMDError <: Exception
    code::Cint
    msg::String
end

function check(ctx::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:cfmm_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
    rc == -1 && throw(ArgumentError(msg))          # CFMM_ERR_INVALID_ARG == the reference's ArgumentError
    throw(CFMMAMDError(rc, msg))
end

# Same readable fields as CFMMRouter.Router (src/router.jl:4-10): objective, cfmms, Δs, Λs, v.
mutable struct AMDRouter{O,T}
    objective::O
    cfmms::Vector{CFMM{T}}
    Δs::Vector{Vector{T}}
    Λs::Vector{Vector{T}}
    v::Vector{T}
    ctx::Ptr{Cvoid}
    order::Vector{Int}          # packed position -> index into cfmms (pools are grouped by family)
    Ψ::Vector{T}
    acc::Base.RefValue{T}
    host::Vector{Int}           # indices of pools whose TYPE has no device kernel: evaluated by their own find_arb! on the host
end

# Router(objective, cfmms, n_tokens) -- src/router.jl:18-36
# `device` is a HIP ordinal, or a vector of ordinals: the pools are then split in contiguous blocks over
# those GPUs from this one Julia task (cfmm_ctx_create_multi: one L-BFGS-B drives all shards, the
# shards' Ψ are summed on the host in device order; no MPI, no RCCL, nothing else to set up).
function AMDRouter(objective::O, cfmms::Vector{C}, n_tokens; device=0) where {O<:Objective,C<:CFMM{Float64}}
    ctxref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if device isa Integer
        ccall((:cfmm_ctx_create, LIB), Cint, (Cint, Int32, Ref{Ptr{Cvoid}}), device, n_tokens, ctxref)
    else
        ids = Int32.(collect(device))
        GC.@preserve ids ccall((:cfmm_ctx_create_multi, LIB), Cint, (Int32, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                               length(ids), ids, n_tokens, ctxref)
    end
    check(Ptr{Cvoid}(C_NULL), rc)
    ctx = ctxref[]
    try
        return build_router(objective, cfmms, n_tokens, ctx)
    catch
        ccall((:cfmm_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), ctx)    # a refused upload (ArgumentError) must not leak the device context
        rethrow()
    end
end

function build_router(objective::O, cfmms::Vector{C}, n_tokens, ctx::Ptr{Cvoid}) where {O<:Objective,C<:CFMM{Float64}}
    order = Int[]
    # --- ProductTwoCoin segment (src/cfmms.jl:101-111) ---
    idx = findall(c -> c isa ProductTwoCoin, cfmms)
    if !isempty(idx)
        R = Float64[c.R[j] for j in 1:2, c in cfmms[idx]]            # 2×m column-major == [m][2] row-major
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:2, c in cfmms[idx]]        # 1-based -> 0-based
        GC.@preserve R γ Ai check(ctx, ccall((:cfmm_pools_add_product, LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ctx, length(idx), R, γ, Ai))
        append!(order, idx)
    end
    # --- GeometricMeanTwoCoin segment (src/cfmms.jl:152-165) ---
    idx = findall(c -> c isa GeometricMeanTwoCoin, cfmms)
    if !isempty(idx)
        R = Float64[c.R[j] for j in 1:2, c in cfmms[idx]]
        w = Float64[c.w[j] for j in 1:2, c in cfmms[idx]]
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:2, c in cfmms[idx]]
        GC.@preserve R w γ Ai check(ctx, ccall((:cfmm_pools_add_geomean, LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ctx, length(idx), R, w, γ, Ai))
        append!(order, idx)
    end
    # --- UniV3 segment, ticks in CSR form (src/cfmms.jl:226-245) ---
    idx = findall(c -> c isa UniV3, cfmms)
    if !isempty(idx)
        cp = Float64[c.current_price for c in cfmms[idx]]
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:2, c in cfmms[idx]]
        off = Int64[0; cumsum(length(c.lower_ticks) for c in cfmms[idx])]
        ticks = reduce(vcat, (Float64.(c.lower_ticks) for c in cfmms[idx]))
        liq = reduce(vcat, (Float64.(c.liquidity) for c in cfmms[idx]))
        GC.@preserve cp γ Ai off ticks liq check(ctx, ccall((:cfmm_pools_add_univ3, LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
            ctx, length(idx), cp, γ, Ai, off, ticks, liq))
        append!(order, idx)
    end
    # --- Solidly stable pairs (φ = R₁³R₂ + R₁R₂³; this module's own type): ProductTwoCoin's arrays ---
    idx = findall(c -> c isa SolidlyStableTwoCoin, cfmms)
    if !isempty(idx)
        R = Float64[c.R[j] for j in 1:2, c in cfmms[idx]]
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:2, c in cfmms[idx]]
        GC.@preserve R γ Ai check(ctx, ccall((:cfmm_pools_add_solidly, LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ctx, length(idx), R, γ, Ai))
        append!(order, idx)
    end
    # --- N-coin GeometricMean / Product pools (src/cfmms.jl:56-63): one weighted segment per coin count ---
    for n in 2:8
        idx = findall(c -> (c isa GeometricMean || c isa Product) && length(c.Ai) == n, cfmms)
        isempty(idx) && continue
        R = Float64[c.R[j] for j in 1:n, c in cfmms[idx]]            # n×m column-major == [m][n] row-major
        w = Float64[c isa Product ? 1.0 : c.w[j] for j in 1:n, c in cfmms[idx]]   # Product: equal weights
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:n, c in cfmms[idx]]
        GC.@preserve R w γ Ai check(ctx, ccall((:cfmm_pools_add_weighted, LIB), Cint,
            (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ctx, length(idx), Int32(n), R, w, γ, Ai))
        append!(order, idx)
    end
    # --- Curve pools (src/cfmms.jl:66-70; φ = α·ΣR − β·ΠR⁻¹, StableSwap at fixed D): one segment per coin count ---
    for n in 2:8
        idx = findall(c -> c isa Curve && length(c.Ai) == n, cfmms)
        isempty(idx) && continue
        R = Float64[c.R[j] for j in 1:n, c in cfmms[idx]]            # n×m column-major == [m][n] row-major
        γ = Float64[c.γ for c in cfmms[idx]]
        Ai = Int32[c.Ai[j] - 1 for j in 1:n, c in cfmms[idx]]
        α = Float64[c.α for c in cfmms[idx]]
        β = Float64[c.β for c in cfmms[idx]]
        GC.@preserve R γ Ai α β check(ctx, ccall((:cfmm_pools_add_curve, LIB), Cint,
            (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
            ctx, length(idx), Int32(n), R, γ, Ai, α, β))
        append!(order, idx)
    end
    # The reference's plugin seam (src/cfmms.jl:35,56; src/router.jl:40): a Router takes ANY CFMM{T} subtype that has a
    # find_arb!(Δ, Λ, cfmm, v) method.  Pools of such a type are not uploaded: every evaluation calls the user's own method
    # on the host and adds its (Λ − Δ) and dual term to what the device returns (host_part! below).
    host = setdiff(1:length(cfmms), order)
    for i in host
        hasmethod(CFMMRouter.find_arb!, Tuple{Vector{Float64},Vector{Float64},typeof(cfmms[i]),Vector{Float64}}) ||
            throw(ArgumentError("cfmms[$i]::$(typeof(cfmms[i])) has no device kernel and no find_arb!(Δ, Λ, cfmm, v) method"))
    end
    Δs = [CFMMRouter.zerotrade(c) for c in cfmms]; Λs = [CFMMRouter.zerotrade(c) for c in cfmms]    # src/router.jl:23-26
    r = AMDRouter{O,Float64}(objective, convert(Vector{CFMM{Float64}}, cfmms), Δs, Λs, zeros(n_tokens), ctx, order,
                             zeros(n_tokens), Ref(0.0), collect(host))
    finalizer(x -> ccall((:cfmm_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.ctx), r)
    return r
end

# Pools without a device kernel: the user's find_arb! per pool (src/router.jl:40), their part of Ψ (src/router.jl:98-100)
# and of the dual scalar (:82) added to the device's
function host_part!(r::AMDRouter, v)
    for i in r.host
        c = r.cfmms[i]
        vl = v[c.Ai]
        CFMMRouter.find_arb!(r.Δs[i], r.Λs[i], c, vl)
        r.acc[] += sum(r.Λs[i] .* vl) - sum(r.Δs[i] .* vl)
        r.Ψ[c.Ai] .+= r.Λs[i] .- r.Δs[i]
    end
    return nothing
end

# r.Δs / r.Λs from the device (cfmm_get_trades): flat, segment after segment, length(c.Ai) values per pool -- r.order lists
# the pools in that segment order
function fetch_trades!(r::AMDRouter)
    len = ccall((:cfmm_trades_len, LIB), Int64, (Ptr{Cvoid},), r.ctx)
    D = Vector{Float64}(undef, len); L = Vector{Float64}(undef, len)
    GC.@preserve D L check(r.ctx, ccall((:cfmm_get_trades, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), r.ctx, D, L))
    off = 0
    for i in r.order
        n = length(r.cfmms[i].Ai)
        r.Δs[i] .= @view D[off+1:off+n]; r.Λs[i] .= @view L[off+1:off+n]
        off += n
    end
    return nothing
end

# find_arb!(r::Router, v) -- src/router.jl:38-42: materialising device sweep, then r.Δs/r.Λs are filled
function find_arb!(r::AMDRouter, v)
    vv = Vector{Float64}(v)
    GC.@preserve vv check(r.ctx, ccall((:cfmm_find_arb, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), r.ctx, vv))
    fetch_trades!(r)
    check(r.ctx, ccall((:cfmm_netflows, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), r.ctx, r.Ψ))
    check(r.ctx, ccall((:cfmm_dual_value, LIB), Cint, (Ptr{Cvoid}, Ref{Float64}), r.ctx, r.acc))
    host_part!(r, vv)
    return nothing
end

# the fused evaluation used inside fn/g! (no O(m) trade write-back)
function eval_pools!(r::AMDRouter, v)
    vv = Vector{Float64}(v)
    GC.@preserve vv check(r.ctx, ccall((:cfmm_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                                       r.ctx, vv, r.Ψ, r.acc))
    host_part!(r, vv)
    return nothing
end

# route!(r; ...) -- src/router.jl:58-108, line for line, with the two O(m) loops replaced by Ψ/acc
function route!(r::AMDRouter; v=nothing, verbose=false, m=5, factr=1e1, pgtol=1e-5, maxfun=15_000, maxiter=15_000)
    optimizer = L_BFGS_B(length(r.v), 17)
    if isnothing(v)
        r.v .= ones(length(r.v)) / length(r.v)
    else
        r.v .= v
    end
    bounds = zeros(3, length(r.v))
    bounds[1, :] .= 2
    bounds[2, :] .= CFMMRouter.lower_limit(r.objective)
    bounds[3, :] .= CFMMRouter.upper_limit(r.objective)

    function fn(v)
        if !all(v .== r.v)
            eval_pools!(r, v)
            r.v .= v
        end
        return CFMMRouter.f(r.objective, v) + r.acc[]          # src/router.jl:79-85
    end
    function g!(G, v)
        G .= 0
        if !all(v .== r.v)
            eval_pools!(r, v)
            r.v .= v
        end
        CFMMRouter.grad!(G, r.objective, v)
        G .+= r.Ψ                                               # src/router.jl:98-100
    end

    eval_pools!(r, r.v)                                         # src/router.jl:104
    _, vopt = optimizer(fn, g!, r.v, bounds, m=m, factr=factr, pgtol=pgtol, iprint=verbose ? 1 : -1,
                        maxfun=maxfun, maxiter=maxiter)
    r.v .= vopt
    find_arb!(r, vopt)                                          # src/router.jl:107
end

# update_pools!(r, changes): new state for a few pools WITHOUT re-uploading the market -- the reference's `cfmm.R .= ...` on some
# pools followed by another route!.  `changes` maps positions in r.cfmms to a reserve vector (two-coin and weighted pools),
# a tuple (R, α, β) (Curve), a price (UniV3; ticks and liquidity stay) or a tuple (price, lower_ticks, liquidity) (UniV3: a
# mint / burn, the pool's new ladder).  The pools are grouped by device segment; every
# segment's rows go through one cfmm_pools_set_* call, which checks all of them before anything changes.  The host-side pool
# objects follow.  Host-evaluated pool types are updated on the host only (their R).
function update_pools!(r::AMDRouter, changes::AbstractDict)
    segs = Dict{Int32,Vector{Tuple{Int64,Int,Any}}}()     # segment => (row, router index, state)
    seg, pos = Int32(0), 0
    groups = Vector{Vector{Int}}()
    for T in (ProductTwoCoin, GeometricMeanTwoCoin, UniV3, SolidlyStableTwoCoin)
        idx = [i for i in r.order[pos+1:end] if r.cfmms[i] isa T]   # r.order is grouped by family
        isempty(idx) && continue
        push!(groups, idx); pos += length(idx)
    end
    for curve in (false, true), n in 2:8
        idx = [i for i in r.order[pos+1:end] if (curve ? r.cfmms[i] isa Curve :
                                                 (r.cfmms[i] isa GeometricMean || r.cfmms[i] isa Product)) &&
                                                length(r.cfmms[i].Ai) == n]
        isempty(idx) && continue
        push!(groups, idx); pos += length(idx)
    end
    where = Dict{Int,Tuple{Int32,Int64}}()
    for (s, idx) in enumerate(groups), (k, i) in enumerate(idx)
        where[i] = (Int32(s - 1), Int64(k - 1))
    end
    for (i, state) in changes
        if i in r.host
            r.cfmms[i].R .= state
            continue
        end
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        s, row = where[i]
        push!(get!(segs, s, Tuple{Int64,Int,Any}[]), (row, i, state))
    end
    for s in sort(collect(keys(segs)))
        items = segs[s]
        idx = Int64[t[1] for t in items]
        c1 = r.cfmms[items[1][2]]
        if c1 isa UniV3 && any(t -> t[3] isa Tuple, items)
            # a mint / burn: (price, lower_ticks, liquidity); every row of the segment goes through ONE call (a bare price
            # with the pool's own ladder), so they are checked together
            p = Float64[Float64(t[3] isa Tuple ? t[3][1] : t[3]) for t in items]
            lts = [Float64.(t[3] isa Tuple ? t[3][2] : r.cfmms[t[2]].lower_ticks) for t in items]
            lqs = [Float64.(t[3] isa Tuple ? t[3][3] : r.cfmms[t[2]].liquidity) for t in items]
            off = Int64[0; cumsum(length.(lts))]
            lt, lq = reduce(vcat, lts), reduce(vcat, lqs)
            GC.@preserve idx p off lt lq check(r.ctx, ccall((:cfmm_pools_set_ticks, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                r.ctx, s, length(idx), idx, p, off, lt, lq))
            for (k, t) in enumerate(items)
                c = r.cfmms[t[2]]
                r.cfmms[t[2]] = UniV3(p[k], lts[k], lqs[k], c.γ, c.Ai)
            end
        elseif c1 isa UniV3
            p = Float64[Float64(t[3]) for t in items]
            GC.@preserve idx p check(r.ctx, ccall((:cfmm_pools_set_prices, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Float64}), r.ctx, s, length(idx), idx, p))
            for (k, t) in enumerate(items)
                c = r.cfmms[t[2]]
                r.cfmms[t[2]] = UniV3(p[k], c.lower_ticks, c.liquidity, c.γ, c.Ai)   # re-derives current_tick (:235)
            end
        elseif c1 isa Curve
            R = reduce(hcat, [Float64.(t[3][1]) for t in items])        # [n_coins, count] column-major = [count][n_coins]
            α = Float64[Float64(t[3][2]) for t in items]
            β = Float64[Float64(t[3][3]) for t in items]
            GC.@preserve idx R α β check(r.ctx, ccall((:cfmm_pools_set_curve, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), r.ctx, s, length(idx), idx, R, α, β))
            for (k, t) in enumerate(items)
                c = r.cfmms[t[2]]
                r.cfmms[t[2]] = Curve(R[:, k], c.γ, c.Ai, α[k], β[k])
            end
        else
            R = reduce(hcat, [Float64.(t[3]) for t in items])
            GC.@preserve idx R check(r.ctx, ccall((:cfmm_pools_set_reserves, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Float64}), r.ctx, s, length(idx), idx, R))
            for (k, t) in enumerate(items)
                r.cfmms[t[2]].R .= @view R[:, k]
            end
        end
    end
    for i in eachindex(r.Δs)      # the trades are those of the old market
        r.Δs[i] .= 0
        r.Λs[i] .= 0
    end
    return nothing
end

# update_reserves!(r) -- src/router.jl:127-132 (upstream calls a per-pool method that exists nowhere).  Here:
# the pools move to R + γΔ − Λ (src/cfmms.jl:26-31) in place on the device, from the trades of the latest
# find_arb!/route!; UniV3 pools move to the price the arbitrage left them at.  The host-side pool objects
# are refreshed from the device (16 bytes per two-coin pool, 8 per UniV3 pool); `sync=false` skips that.
function update_reserves!(r::AMDRouter; sync::Bool=true)
    for i in r.host      # host-evaluated pool types: their own per-pool method, as src/router.jl:129 calls it
        CFMMRouter.update_reserves!(r.cfmms[i], r.Δs[i], r.Λs[i], r.v[r.cfmms[i].Ai])
    end
    check(r.ctx, ccall((:cfmm_update_reserves, LIB), Cint, (Ptr{Cvoid},), r.ctx))
    sync && download_state!(r)
    foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    return nothing
end

# the host-side pool objects <- the device: reserves of every reserve kind, current prices of the UniV3 pools
function download_state!(r::AMDRouter)
    seg, pos = Int32(0), 0
    for T in (ProductTwoCoin, GeometricMeanTwoCoin, UniV3, SolidlyStableTwoCoin)
        idx = [i for i in r.order[pos+1:end] if r.cfmms[i] isa T]   # r.order is grouped by family
        isempty(idx) && continue
        if T === UniV3
            p = Vector{Float64}(undef, length(idx))
            GC.@preserve p check(r.ctx, ccall((:cfmm_get_prices, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), r.ctx, seg, p))
            for (k, i) in enumerate(idx)
                c = r.cfmms[i]
                r.cfmms[i] = UniV3(p[k], c.lower_ticks, c.liquidity, c.γ, c.Ai)   # re-derives current_tick (:235)
            end
        else
            R = Matrix{Float64}(undef, 2, length(idx))
            GC.@preserve R check(r.ctx, ccall((:cfmm_get_reserves, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), r.ctx, seg, R))
            for (k, i) in enumerate(idx)
                r.cfmms[i].R .= @view R[:, k]
            end
        end
        seg += Int32(1); pos += length(idx)
    end
    # weighted segments follow, one per coin count, then Curve segments (build_router); Curve's α, β stay
    for curve in (false, true), n in 2:8
        idx = [i for i in r.order[pos+1:end] if (curve ? r.cfmms[i] isa Curve :
                                                 (r.cfmms[i] isa GeometricMean || r.cfmms[i] isa Product)) &&
                                                length(r.cfmms[i].Ai) == n]
        isempty(idx) && continue
        R = Matrix{Float64}(undef, n, length(idx))
        GC.@preserve R check(r.ctx, ccall((:cfmm_get_reserves, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), r.ctx, seg, R))
        for (k, i) in enumerate(idx)
            r.cfmms[i].R .= @view R[:, k]
        end
        seg += Int32(1); pos += length(idx)
    end
    return nothing
end

# select_trades(r, seg; min_value, v, capacity): the pools of device segment `seg` (0-based, the order of build_router) that
# trade in the latest find_arb! / route! and are worth at least min_value, compacted on the device (cfmm_select_trades):
# a pool trades iff some entry of its Δ or Λ compares != 0.0, value = Σ_k (Λ_k − Δ_k)·v[A_k] in coin order, selected unless
# value < min_value.  -> (idx, Δ, Λ, value): idx = 1-based rows within the segment, ascending; Δ, Λ = n_coins × count matrices
# (column j = the trade of pool idx[j]).  v = nothing: the prices of that sweep.  capacity = nothing: min(m, 65536) rows
# first, then once more with the returned count if that was too small.
function select_trades(r::AMDRouter, seg::Integer; min_value::Real=0.0, v=nothing, capacity=nothing, n_coins::Integer=2)
    isnothing(capacity) || capacity >= 0 || throw(ArgumentError("capacity must be >= 0"))
    vv = isnothing(v) ? Float64[] : Vector{Float64}(v)
    cap = isnothing(capacity) ? 65536 : Int64(capacity)
    while true
        idx = Vector{Int64}(undef, cap); val = Vector{Float64}(undef, cap)
        D = Matrix{Float64}(undef, n_coins, cap); L = Matrix{Float64}(undef, n_coins, cap)
        count = Ref{Int64}(0)
        GC.@preserve vv idx val D L check(r.ctx, ccall((:cfmm_select_trades, LIB), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Float64}, Float64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            r.ctx, Int32(seg), isnothing(v) ? C_NULL : pointer(vv), Float64(min_value), cap, count, idx, D, L, val))
        if count[] <= cap || !isnothing(capacity)
            k = min(count[], cap)
            return idx[1:k] .+ 1, D[:, 1:k], L[:, 1:k], val[1:k]
        end
        cap = count[]
    end
end

# Device segment and 0-based row of every device pool of the router: the order of build_router (r.order grouped by family,
# then weighted pools per coin count, then Curve pools per coin count), derived as update_pools! derives it (that function
# keeps its own copy: it is left as it was).
function segment_rows(r::AMDRouter)
    pos = 0
    groups = Vector{Vector{Int}}()
    for T in (ProductTwoCoin, GeometricMeanTwoCoin, UniV3, SolidlyStableTwoCoin)
        idx = [i for i in r.order[pos+1:end] if r.cfmms[i] isa T]
        isempty(idx) && continue
        push!(groups, idx); pos += length(idx)
    end
    for curve in (false, true), n in 2:8
        idx = [i for i in r.order[pos+1:end] if (curve ? r.cfmms[i] isa Curve :
                                                 (r.cfmms[i] isa GeometricMean || r.cfmms[i] isa Product)) &&
                                                length(r.cfmms[i].Ai) == n]
        isempty(idx) && continue
        push!(groups, idx); pos += length(idx)
    end
    where = Dict{Int,Tuple{Int32,Int64}}()
    for (s, idx) in enumerate(groups), (k, i) in enumerate(idx)
        where[i] = (Int32(s - 1), Int64(k - 1))
    end
    return where
end

# quote_swaps(r, pools, coin_in, amount_in; coin_out) -- the Python host's router-level `quote` (a reserved word here): exact-input swap quotes on the pools as they stand on the device (cfmm_quote;
# forward_trade, src/cfmms.jl:436-449, for every device kind): what comes out of pool pools[q] (positions in r.cfmms, any
# order, repeats allowed) for amount_in[q] of its coin coin_in[q] (1-based positions in the pool's own coin order).
# coin_out = nothing: the other coin of a two-coin or UniV3 pool.  Each segment's queries go through one call; the results
# return in the caller's order.  Read-only.  A host-evaluated pool type has no device state to quote: ArgumentError.
function quote_swaps(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                     amount_in::AbstractVector{<:Real}; coin_out=nothing)
    return quote_queries(r, pools, coin_in, amount_in, coin_out, false)
end

# quote_swaps_out(r, pools, coin_in, amount_out; coin_out) -- the inverse (cfmm_quote_out; the Python host's `quote_out`): how
# much of its coin coin_in[q] pool pools[q] must be tendered so that exactly amount_out[q] of the coin out comes from it as it
# stands on the device; Inf where the pool cannot give that much.  Arguments, mapping and order as quote_swaps.
function quote_swaps_out(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                         amount_out::AbstractVector{<:Real}; coin_out=nothing)
    return quote_queries(r, pools, coin_in, amount_out, coin_out, true)
end

# swap!(r, pools, coin_in, amount_in; coin_out) -- the Python host's `swap_` (cfmm_swap): quote_swaps' arguments, but every swap
# is APPLIED.  The swaps of a segment go through one call in the caller's order, so a pool named k times is swapped k times,
# each from the state the previous one left; amount_out[q] is what quote_swaps answers on the pool as the earlier swaps left
# it, and the pool then moves to R + γΔ − Λ (UniV3: to the price the swap rests at).  A swap that would leave an invalid pool
# is not applied and answers NaN.  sync = true refreshes the host-side pool objects; the router's trades are those of the old
# market and are zeroed, as by update_pools!.
function swap!(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
               amount_in::AbstractVector{<:Real}; coin_out=nothing, sync::Bool=true)
    n = length(pools)
    (length(coin_in) == n && length(amount_in) == n && (isnothing(coin_out) || length(coin_out) == n)) ||
        throw(ArgumentError("coin_in, the amounts and coin_out must have one entry per pool"))
    where = segment_rows(r)
    segs = Dict{Int32,Vector{Int}}()                      # segment => query numbers, in the caller's order
    for (q, i) in enumerate(pools)
        i in r.host && throw(ArgumentError("pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        push!(get!(segs, where[i][1], Int[]), q)
    end
    out = Vector{Float64}(undef, n)
    try
        for s in sort(collect(keys(segs)))
            qs = segs[s]
            idx = Int64[where[pools[q]][2] for q in qs]
            ci = Int32[coin_in[q] - 1 for q in qs]
            co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
            amt = Float64[amount_in[q] for q in qs]
            res = Vector{Float64}(undef, length(qs))
            cop = isnothing(coin_out) ? C_NULL : pointer(co)
            GC.@preserve idx ci co amt res check(r.ctx,
                ccall((:cfmm_swap, LIB), Cint,
                      (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                      r.ctx, s, length(qs), idx, ci, cop, amt, res))
            out[qs] .= res
        end
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return out
end

# swap_out!(r, pools, coin_in, amount_out; coin_out, max_in=nothing, sync=true) -- the Python host's `swap_out_` (cfmm_swap_out):
# quote_swaps_out's arguments, but every swap is APPLIED: the pool gives exactly amount_out[q] and takes what quote_swaps_out
# answers on the pool as the earlier swaps of the call left it (R_in + γ·amount_in, R_out − amount_out; UniV3: the price swap!
# of amount_in rests at).  Returns (amount_in, status): status[q] is 0 (applied), 3 (the pool cannot give that much: Inf),
# 2 (the swap would leave an invalid pool: NaN) or 1 (amount_in[q] > max_in[q]: the quote it would have cost); in the last
# three the pool stays as it was.  Order within a segment, sync and the zeroing of the router's trades are swap!'s.
const SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE = Int32(0), Int32(1), Int32(2), Int32(3)   # CFMM_SWAP_*
function swap_out!(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                   amount_out::AbstractVector{<:Real}; coin_out=nothing, max_in=nothing, sync::Bool=true)
    n = length(pools)
    (length(coin_in) == n && length(amount_out) == n && (isnothing(coin_out) || length(coin_out) == n) &&
     (isnothing(max_in) || length(max_in) == n)) ||
        throw(ArgumentError("coin_in, the amounts, coin_out and max_in must have one entry per pool"))
    where = segment_rows(r)
    segs = Dict{Int32,Vector{Int}}()                      # segment => query numbers, in the caller's order
    for (q, i) in enumerate(pools)
        i in r.host && throw(ArgumentError("pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        push!(get!(segs, where[i][1], Int[]), q)
    end
    out = Vector{Float64}(undef, n)
    status = Vector{Int32}(undef, n)
    try
        for s in sort(collect(keys(segs)))
            qs = segs[s]
            idx = Int64[where[pools[q]][2] for q in qs]
            ci = Int32[coin_in[q] - 1 for q in qs]
            co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
            amt = Float64[amount_out[q] for q in qs]
            lim = isnothing(max_in) ? Float64[] : Float64[max_in[q] for q in qs]
            res = Vector{Float64}(undef, length(qs))
            st = Vector{Int32}(undef, length(qs))
            cop = isnothing(coin_out) ? C_NULL : pointer(co)
            lp = isnothing(max_in) ? Ptr{Float64}(C_NULL) : pointer(lim)
            GC.@preserve idx ci co amt lim res st check(r.ctx,
                ccall((:cfmm_swap_out, LIB), Cint,
                      (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                      r.ctx, s, length(qs), idx, ci, cop, amt, lp, res, st))
            out[qs] .= res
            status[qs] .= st
        end
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return out, status
end

# both directions: `amount_in` is the GIVEN amount (the wanted output when exact_out), the result the answer
function quote_queries(r::AMDRouter, pools, coin_in, amount_in, coin_out, exact_out::Bool)
    n = length(pools)
    (length(coin_in) == n && length(amount_in) == n && (isnothing(coin_out) || length(coin_out) == n)) ||
        throw(ArgumentError("coin_in, the amounts and coin_out must have one entry per pool"))
    where = segment_rows(r)
    segs = Dict{Int32,Vector{Int}}()                      # segment => query numbers
    for (q, i) in enumerate(pools)
        i in r.host && throw(ArgumentError("pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        push!(get!(segs, where[i][1], Int[]), q)
    end
    out = Vector{Float64}(undef, n)
    for s in sort(collect(keys(segs)))
        qs = segs[s]
        idx = Int64[where[pools[q]][2] for q in qs]
        ci = Int32[coin_in[q] - 1 for q in qs]
        co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
        amt = Float64[amount_in[q] for q in qs]
        res = Vector{Float64}(undef, length(qs))
        cop = isnothing(coin_out) ? C_NULL : pointer(co)
        GC.@preserve idx ci co amt res check(r.ctx, exact_out ?
            ccall((:cfmm_quote_out, LIB), Cint,
                  (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                  r.ctx, s, length(qs), idx, ci, cop, amt, res) :
            ccall((:cfmm_quote, LIB), Cint,
            (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
            r.ctx, s, length(qs), idx, ci, cop, amt, res))
        out[qs] .= res
    end
    return out
end

# quote_paths(r, pools, tokens, amount_in; hops=false) -- the Python host's router-level `quote_path` (cfmm_quote_path): amount_in[p]
# of token tokens[p][1] carried through the pools pools[p] (1 .. 8 positions in r.cfmms) in one launch, whatever kinds they
# are: hop k trades tokens[p][k] for tokens[p][k+1] (token ids as in Ai, one more than the pools).  EVERY HOP IS QUOTED
# AGAINST THE POOL AS IT STANDS -- no state advances between hops -- so a pool may appear only once in a path.  The coin
# positions are found in the pool's Ai and converted to the library's 0-based ones here.  ArgumentError, naming path and
# hop, for a token that is not a coin of the pool or is the same on both sides, a repeated pool, a host-evaluated pool,
# more than 8 pools.  hops=true: also the [count, max_hops] amounts leaving each hop (NaN where a path has no such hop).
function quote_paths(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_in::AbstractVector{<:Real}; hops::Bool=false)
    return quote_path_queries(r, pools, tokens, amount_in, hops, false)
end

# quote_paths_out(r, pools, tokens, amount_out; hops=false) -- the inverse (cfmm_quote_path_out): what to tender to the first pool
# so that exactly amount_out[p] leaves the last, walked from the last hop backwards; Inf where a pool on the way cannot give
# that much.  hops=true: also the amounts to tender to each hop.
function quote_paths_out(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_out::AbstractVector{<:Real}; hops::Bool=false)
    return quote_path_queries(r, pools, tokens, amount_out, hops, true)
end

const MAX_PATH_HOPS = 8   # CFMM_MAX_PATH_HOPS

# (pools, tokens) of the path calls as the library's hop arrays, with every refusal made here
function path_hop_arrays(r::AMDRouter, pools, tokens, given)
    n = length(pools)
    (length(tokens) == n && length(given) == n) || throw(ArgumentError("tokens and the amounts must have one entry per path"))
    where = segment_rows(r)
    H = max(1, maximum(length, pools; init=1))
    n_hops = Int32[length(p) for p in pools]
    seg = zeros(Int32, n, H); ci = zeros(Int32, n, H); co = zeros(Int32, n, H)     # column-major [count, max_hops] IS the
    row = zeros(Int64, n, H)                                                       # library's hop-major layout
    for p in 1:n
        1 <= length(pools[p]) <= MAX_PATH_HOPS || throw(ArgumentError("path $p: $(length(pools[p])) pools (a path has 1 to $MAX_PATH_HOPS)"))
        length(tokens[p]) == length(pools[p]) + 1 || throw(ArgumentError("path $p: $(length(tokens[p])) tokens for $(length(pools[p])) pools"))
        for (k, i) in enumerate(pools[p])
            i in r.host && throw(ArgumentError("path $p, hop $k: pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
            haskey(where, i) || throw(ArgumentError("path $p, hop $k: pool $i out of range"))
            i in pools[p][1:k-1] && throw(ArgumentError("path $p, hop $k: pool $i appears twice (every hop is quoted against the pool as it stands)"))
            a = findfirst(==(tokens[p][k]), r.cfmms[i].Ai)
            b = findfirst(==(tokens[p][k+1]), r.cfmms[i].Ai)
            (isnothing(a) || isnothing(b)) && throw(ArgumentError("path $p, hop $k: token $(isnothing(a) ? tokens[p][k] : tokens[p][k+1]) is not a coin of pool $i"))
            a == b && throw(ArgumentError("path $p, hop $k: token $(tokens[p][k]) on both sides of pool $i"))
            seg[p, k], row[p, k] = where[i]
            ci[p, k] = a - 1; co[p, k] = b - 1                                      # 0-based for the library
        end
    end
    return n, H, n_hops, seg, row, ci, co, Float64[given[p] for p in 1:n]
end

function quote_path_queries(r::AMDRouter, pools, tokens, given, hops::Bool, exact_out::Bool)
    n, H, n_hops, seg, row, ci, co, amt = path_hop_arrays(r, pools, tokens, given)
    out = Vector{Float64}(undef, n)
    hv = fill(NaN, n, H)
    n == 0 && return hops ? (out, hv) : out
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    GC.@preserve n_hops seg row ci co amt out hv check(r.ctx, exact_out ?
        ccall((:cfmm_quote_path_out, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              r.ctx, n, H, n_hops, seg, row, ci, co, amt, out, hp) :
        ccall((:cfmm_quote_path, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              r.ctx, n, H, n_hops, seg, row, ci, co, amt, out, hp))
    return hops ? (out, hv) : out
end

# swap_paths!(r, pools, tokens, amount_in; min_out=nothing, hops=false, sync=true) -- the Python host's `swap_path_`
# (cfmm_swap_path): quote_paths' arguments, mapping and refusals, but the paths are EXECUTED in the order given, each all or
# nothing.  Path p sees the market as the applied paths before it left it; an applied path's amounts are what quote_paths
# answers on that market and each of its pools moves as swap! moves it.  Returns (amount_out, status[, hop_out]): status[p]
# is 0 (applied), 1 (amount_out[p] < min_out[p]: the quote it would have given, nothing moved) or 2 (a hop would leave an
# invalid pool: NaN, nothing moved).  sync = true refreshes the host-side pool objects; the router's trades are zeroed.
const PATH_APPLIED, PATH_BELOW_LIMIT, PATH_REFUSED = Int32(0), Int32(1), Int32(2)   # CFMM_PATH_*
function swap_paths!(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_in::AbstractVector{<:Real};
                     min_out=nothing, hops::Bool=false, sync::Bool=true)
    n, H, n_hops, seg, row, ci, co, amt = path_hop_arrays(r, pools, tokens, amount_in)
    (isnothing(min_out) || length(min_out) == n) || throw(ArgumentError("min_out must have one entry per path"))
    lim = isnothing(min_out) ? Float64[] : Float64[min_out[p] for p in 1:n]
    out = Vector{Float64}(undef, n)
    status = Vector{Int32}(undef, n)
    hv = fill(NaN, n, H)
    n == 0 && return hops ? (out, status, hv) : (out, status)
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    lp = isnothing(min_out) ? Ptr{Float64}(C_NULL) : pointer(lim)
    try
        GC.@preserve n_hops seg row ci co amt lim out hv status check(r.ctx,
            ccall((:cfmm_swap_path, LIB), Cint,
                  (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  r.ctx, n, H, n_hops, seg, row, ci, co, amt, lp, out, hp, status))
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return hops ? (out, status, hv) : (out, status)
end


# find_paths(r, token_in, token_out, amount_in; max_hops=3) -- the Python host's router-level `find_path` (cfmm_find_path): the
# best swap path of at most max_hops (1 .. 8) pools from token_in[q] to token_out[q] (token ids as in Ai) for amount_in[q],
# FOUND on the device among the pools as they stand there.  Returns (amount_out, pools, tokens, status): pools[q] / tokens[q]
# in the form quote_paths / swap_paths! take (positions in r.cfmms; the tokens along the path, one more than the pools), empty
# where nothing was found.  The contract is the layered search: layer h holds per token the largest quote over every pool and
# ordered coin pair from layer h-1, every hop quoted against the pool as it stands; the answer is the largest layer entry of
# token_out with the fewest hops, ties to the smallest (segment, row, coin_in, coin_out) -- quote_paths on the result answers
# amount_out bit for bit.  What is found is a walk: status[q] is 0 (found), 1 (token_out not reached within max_hops, or
# amount 0: amount_out 0.0) or 2 (found, but the walk visits a pool twice: quote_paths and swap_paths! refuse it as one
# path).  Host-evaluated pools have no device state and are not searched.  Read-only.
const FOUND, FOUND_NONE, FOUND_REPEATS = Int32(0), Int32(1), Int32(2)   # CFMM_FOUND*
function find_paths(r::AMDRouter, token_in::AbstractVector{<:Integer}, token_out::AbstractVector{<:Integer},
                    amount_in::AbstractVector{<:Real}; max_hops::Integer=3)
    n = length(token_in)
    (length(token_out) == n && length(amount_in) == n) || throw(ArgumentError("token_in, token_out and amount_in must have one entry per query"))
    nt = length(r.v)
    for q in 1:n
        1 <= token_in[q] <= nt || throw(ArgumentError("query $q: token_in $(token_in[q]) out of range 1:$nt"))
        1 <= token_out[q] <= nt || throw(ArgumentError("query $q: token_out $(token_out[q]) out of range 1:$nt"))
    end
    1 <= max_hops <= MAX_PATH_HOPS || throw(ArgumentError("max_hops must be 1 to $MAX_PATH_HOPS"))
    H = Int(max_hops)
    tin = Int32[token_in[q] - 1 for q in 1:n]; tout = Int32[token_out[q] - 1 for q in 1:n]       # 0-based for the library
    amt = Float64[amount_in[q] for q in 1:n]
    out = Vector{Float64}(undef, n)
    n_hops = Vector{Int32}(undef, n); status = Vector{Int32}(undef, n)
    seg = fill(Int32(-1), n, H); ci = fill(Int32(-1), n, H); co = fill(Int32(-1), n, H)          # column-major [count, max_hops] IS the
    row = fill(Int64(-1), n, H)                                                                  # library's hop-major layout
    n == 0 && return out, Vector{Int}[], Vector{Int}[], status
    GC.@preserve tin tout amt out n_hops seg row ci co status check(r.ctx,
        ccall((:cfmm_find_path, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
              r.ctx, n, H, tin, tout, amt, out, n_hops, seg, row, ci, co, status))
    pool_at = Dict{Tuple{Int32,Int64},Int}(sr => i for (i, sr) in segment_rows(r))
    pools = Vector{Vector{Int}}(undef, n); tokens = Vector{Vector{Int}}(undef, n)
    for q in 1:n
        pools[q] = Int[pool_at[(seg[q, k], row[q, k])] for k in 1:n_hops[q]]
        tokens[q] = n_hops[q] == 0 ? Int[] : vcat(Int(token_in[q]), Int[r.cfmms[pools[q][k]].Ai[co[q, k] + 1] for k in 1:n_hops[q]])
    end
    return out, pools, tokens, status
end

include("swap_paths_out.jl")   # swap_paths_out! (cfmm_swap_path_out, declared in include/cfmm_amd_path_out.h)
include("find_paths_out.jl")   # find_paths_out (cfmm_find_path_out, declared in include/cfmm_amd_find_out.h)
include("size_paths.jl")       # size_paths (cfmm_size_path, declared in include/cfmm_amd_size_path.h)
include("split_paths.jl")      # split_paths (cfmm_split_paths, declared in include/cfmm_amd_split.h)
include("find_disjoint_paths.jl")   # find_disjoint_paths (cfmm_find_disjoint_paths, declared in include/cfmm_amd_find_disjoint.h)
include("split_paths_out.jl")      # split_paths_out (cfmm_split_paths_out, declared in include/cfmm_amd_split_out.h)
include("find_disjoint_paths_out.jl")   # find_disjoint_paths_out (cfmm_find_disjoint_paths_out, declared in include/cfmm_amd_find_disjoint_out.h)
include("quote_rate.jl")      # quote_rate, spot_price, quote_path_rate (cfmm_quote_rate, cfmm_quote_path_rate, declared in include/cfmm_amd_rate.h)
include("quote_to_rate.jl")   # amount_to_rate, swap_limit! (cfmm_quote_to_rate, cfmm_swap_limit, declared in include/cfmm_amd_limit.h)
include("swap_order.jl")      # swap_orders!, swap_orders_out! (cfmm_swap_order, cfmm_swap_order_out, declared in include/cfmm_amd_order.h)

# forward_trade(Δ, cfmm) -- src/cfmms.jl:436-449: methods of CFMMRouter's own function (imported above) for the pool kinds it
# has none for, one pool through the device (a one-pool AMDRouter).  Δ has exactly one positive entry; on pools of more than
# two coins the keyword coin_out (1-based) is required.  Δ == 0 returns 0.0 (:440-442).  UniV3 keeps the reference's own
# method (:436): a method here for (AbstractVector, UniV3) would be ambiguous with it or replace it; the device's UniV3 quote
# is quote_swaps on a router that holds the pool.
const DeviceQuotedPool = Union{ProductTwoCoin{Float64},GeometricMeanTwoCoin{Float64},Product{Float64},GeometricMean{Float64},
                               Curve{Float64},SolidlyStableTwoCoin{Float64}}
function forward_trade(Δ::AbstractVector{<:Real}, cfmm::DeviceQuotedPool; coin_out=nothing, device=0)
    n = length(cfmm.Ai)
    length(Δ) == n || throw(ArgumentError("Δ must have $n entries"))
    (all(isfinite, Δ) && all(>=(0), Δ)) || throw(ArgumentError("Δ must be finite and >= 0"))
    pos = findall(>(0), Δ)
    length(pos) <= 1 || throw(ArgumentError("Δ must have exactly one positive entry (one coin in)"))
    (isnothing(coin_out) && n > 2) && throw(ArgumentError("coin_out is required on a pool of $n coins"))
    (isnothing(coin_out) || 1 <= coin_out <= n) || throw(ArgumentError("coin_out $coin_out out of range 1:$n"))
    isempty(pos) && return 0.0
    (!isnothing(coin_out) && coin_out == pos[1]) && throw(ArgumentError("coin_out is the tendered coin"))
    nt = Int(maximum(cfmm.Ai))
    r = AMDRouter(CFMMRouter.LinearNonnegative(ones(nt)), [cfmm], nt; device=device)
    return quote_swaps(r, [1], [pos[1]], [Float64(Δ[pos[1]])]; coin_out=isnothing(coin_out) ? nothing : [coin_out])[1]
end

# backward_trade(Λ, cfmm) -- the mirror of forward_trade (the reference has none): Λ has exactly one positive entry, the amount
# wanted at the position of its coin; returns the amount of the other coin -- of coin coin_in (1-based; required on pools of
# more than two coins) -- that must be tendered, Inf where the pool cannot give Λ.  Λ == 0 returns 0.0.  One pool through the
# device (a one-pool AMDRouter), as forward_trade.
function backward_trade(Λ::AbstractVector{<:Real}, cfmm::DeviceQuotedPool; coin_in=nothing, device=0)
    n = length(cfmm.Ai)
    length(Λ) == n || throw(ArgumentError("Λ must have $n entries"))
    (all(isfinite, Λ) && all(>=(0), Λ)) || throw(ArgumentError("Λ must be finite and >= 0"))
    pos = findall(>(0), Λ)
    length(pos) <= 1 || throw(ArgumentError("Λ must have exactly one positive entry (one coin out)"))
    (isnothing(coin_in) && n > 2) && throw(ArgumentError("coin_in is required on a pool of $n coins"))
    (isnothing(coin_in) || 1 <= coin_in <= n) || throw(ArgumentError("coin_in $coin_in out of range 1:$n"))
    isempty(pos) && return 0.0
    (!isnothing(coin_in) && coin_in == pos[1]) && throw(ArgumentError("coin_in is the wanted coin"))
    cin = isnothing(coin_in) ? 3 - pos[1] : coin_in
    nt = Int(maximum(cfmm.Ai))
    r = AMDRouter(CFMMRouter.LinearNonnegative(ones(nt)), [cfmm], nt; device=device)
    return quote_swaps_out(r, [1], [cin], [Float64(Λ[pos[1]])]; coin_out=[pos[1]])[1]
end

# Optional fast path: the whole of route! inside the library (cfmm_route: its own L-BFGS-B, the
# objective's f/grad!/bounds restated in C++) -- one ccall, no Julia between two device sweeps.
struct RouteInfo
    f::Float64
    proj_grad::Float64
    iterations::Int32
    evaluations::Int32
    sweeps::Int32
    status::Int32
    sweep_seconds::Float64
    total_seconds::Float64
end

function route_native!(r::AMDRouter; v=nothing, m=5, factr=1e1, pgtol=1e-5, maxfun=15_000, maxiter=15_000)
    isempty(r.host) || throw(ArgumentError("route_native! runs inside the library: routers with host-evaluated pool types use route!"))
    obj = r.objective
    kind, vec, idx = if obj isa CFMMRouter.LinearNonnegative
        (Int32(0), Vector{Float64}(obj.c), Int32(0))
    elseif obj isa CFMMRouter.BasketLiquidation
        (Int32(1), Vector{Float64}(obj.Δin), Int32(obj.i - 1))
    else
        throw(ArgumentError("route_native! knows LinearNonnegative and BasketLiquidation"))
    end
    n = length(r.v)
    vout = Vector{Float64}(undef, n)
    info = Ref(RouteInfo(0.0, 0.0, 0, 0, 0, 0, 0.0, 0.0))
    v0vec = isnothing(v) ? Float64[] : Vector{Float64}(v)
    GC.@preserve vec v0vec vout check(r.ctx, ccall((:cfmm_route, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Float64, Float64, Int32, Int32,
         Ptr{Float64}, Ptr{Float64}, Ref{RouteInfo}),
        r.ctx, kind, vec, idx, isnothing(v) ? C_NULL : pointer(v0vec), m, factr, pgtol, maxfun, maxiter,
        vout, r.Ψ, info))
    r.v .= vout
    # trades were materialised at v* by the same call
    fetch_trades!(r)
    return info[]
end

# cfmm_polish (include/cfmm_amd.h): tighten a route!'s result with a gradient-only projected chord-Newton iteration on the
# dual's optimality conditions -- NOT part of CFMMRouter.jl (its route! ends where L-BFGS-B ends, with a stationarity
# residual of ~1e-6 max|Ψ| on interior optima); overwrites r.v, r.Δs, r.Λs like route! does.
struct PolishInfo
    residual0::Float64
    residual::Float64
    iterations::Int32
    sweeps::Int32
    total_seconds::Float64
end

function polish!(r::AMDRouter; max_iters=8, rel_step=1e-7)
    isempty(r.host) || throw(ArgumentError("polish! runs inside the library: not available with host-evaluated pool types"))
    obj = r.objective
    kind, vec, idx = if obj isa CFMMRouter.LinearNonnegative
        (Int32(0), Vector{Float64}(obj.c), Int32(0))
    elseif obj isa CFMMRouter.BasketLiquidation
        (Int32(1), Vector{Float64}(obj.Δin), Int32(obj.i - 1))
    else
        throw(ArgumentError("polish! knows LinearNonnegative and BasketLiquidation"))
    end
    vio = Vector{Float64}(r.v)
    info = Ref(PolishInfo(0.0, 0.0, 0, 0, 0.0))
    GC.@preserve vec vio check(r.ctx, ccall((:cfmm_polish, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ref{PolishInfo}),
        r.ctx, kind, vec, idx, vio, max_iters, rel_step, r.Ψ, info))
    r.v .= vio
    fetch_trades!(r)
    return info[]
end

# Library options (include/cfmm_amd.h, cfmm_set_option): e.g. set_option!(r, "stop_in_noise", 1) for the noise-floor
# stop of route_native! (default 0 = the stopping rules of L-BFGS-B 3.0), set_option!(r, "fast_math", 0), ...
function set_option!(r::AMDRouter, key::AbstractString, value::Integer)
    check(r.ctx, ccall((:cfmm_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), r.ctx, key, Int64(value)))
    return nothing
end

# Sharding over the GPUs of a node, one Julia process per GPU (Distributed.jl workers, MPI.jl ranks ...): north_star's
# "RCCL all-reduce of Ψ and ∇g over xGMI per outer iteration" in three calls (include/cfmm_amd.h, sharded runs through RCCL).
# Every rank builds its AMDRouter over ITS contiguous block of the cfmms vector (the axis of src/router.jl:39) on its own
# device; rank 0 draws the id, the launcher's own channel carries the 128 bytes, every rank joins:
#     id = rank == 0 ? rccl_unique_id() : nothing;  id = MPI.bcast(id, 0, comm)      # or remotecall_fetch / a file
#     rccl_init_rank!(r, id, world, rank)            # collective
# From then on find_arb!(r, v), eval_pools!, route!, route_native! return the Ψ / dual value of the WHOLE market on every
# rank (bit-identical: the ranks' L-BFGS-B stays in lockstep); r.Δs / r.Λs are the local shard's trades.
function rccl_unique_id()
    id = Vector{UInt8}(undef, 128)
    GC.@preserve id check(C_NULL, ccall((:cfmm_rccl_unique_id, LIB), Cint, (Ptr{UInt8},), id))
    return id
end

function rccl_init_rank!(r::AMDRouter, id::Vector{UInt8}, world::Integer, rank::Integer)
    length(id) == 128 || throw(ArgumentError("the id of rccl_unique_id() has 128 bytes"))
    GC.@preserve id check(r.ctx, ccall((:cfmm_rccl_init_rank, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32),
                                       r.ctx, id, Int32(world), Int32(rank)))
    return nothing
end

# a communicator the host created itself (RCCL.jl / a C launcher); C_NULL switches the exchange off
function set_rccl_comm!(r::AMDRouter, comm::Ptr{Cvoid})
    check(r.ctx, ccall((:cfmm_set_rccl_comm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), r.ctx, comm))
    return nothing
end

# netflows!(ψ, r) / netflows(r) -- src/router.jl:111-125.
# exact = true (default): the reference's own loop over r.Δs / r.Λs / r.cfmms in router order (:113-116) -- the rows are on
# the host anyway after find_arb! / route! -- so `all_flows .== netflows(r)` of the reference's router test (test/arb.jl:16)
# holds unedited.  exact = false: the device's reduction of the same sweep (what route! itself consumed as the gradient;
# within 1e-12 max|Ψ| of the serial sum), no O(m) host loop.
function netflows!(ψ, r::AMDRouter; exact::Bool=true)
    if exact
        fill!(ψ, 0)
        for (Δ, Λ, c) in zip(r.Δs, r.Λs, r.cfmms)
            ψ[c.Ai] .+= Λ .- Δ
        end
    else
        ψ .= r.Ψ
    end
    return nothing
end
function netflows(r::AMDRouter; exact::Bool=true)
    ψ = zero(r.v)
    netflows!(ψ, r; exact=exact)
    return ψ
end

end # module
