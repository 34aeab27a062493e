# quote_to_rate.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): price limits, the inverse of quote_rate.
# Its entries, cfmm_quote_to_rate and cfmm_swap_limit, are declared in include/cfmm_amd_limit.h, beside include/cfmm_amd_rate.h.

const LIMIT_FILLED = Int32(0)
const LIMIT_PARTIAL = Int32(1)
const LIMIT_NONE = Int32(2)
const LIMIT_REFUSED = Int32(3)

# pools (positions in r.cfmms) grouped by segment, as quote_rate_queries groups them: segment => query numbers
function limit_segments(r::AMDRouter, pools, columns...)
    n = length(pools)
    all(c -> isnothing(c) || length(c) == n, columns) || throw(ArgumentError("every argument must have one entry per pool"))
    where = segment_rows(r)
    segs = Dict{Int32,Vector{Int}}()
    for (q, i) in enumerate(pools)
        i in r.host && throw(ArgumentError("pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        push!(get!(segs, where[i][1], Int[]), q)
    end
    return where, segs
end

# amount_to_rate(r, pools, coin_in, rate; coin_out) -- the Python host's `Context.quote_to_rate` per pool (cfmm_quote_to_rate):
# quote_rate's arguments with the limit in the place of the amount; returns (amount_in, amount_out).  amount_in[q] is how much
# of coin_in[q] pool pools[q] takes before its marginal rate has fallen to rate[q] -- exactly 0.0 where the spot rate is already
# at or below it -- and amount_out[q] is quote_swaps' answer for it, bit for bit.  rate must be finite and > 0.  Read-only.
function amount_to_rate(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                        rate::AbstractVector{<:Real}; coin_out=nothing)
    where, segs = limit_segments(r, pools, coin_in, rate, coin_out)
    n = length(pools)
    amount = Vector{Float64}(undef, n)
    out = Vector{Float64}(undef, n)
    for s in sort(collect(keys(segs)))
        qs = segs[s]
        idx = Int64[where[pools[q]][2] for q in qs]
        ci = Int32[coin_in[q] - 1 for q in qs]
        co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
        lim = Float64[rate[q] for q in qs]
        a = Vector{Float64}(undef, length(qs))
        o = Vector{Float64}(undef, length(qs))
        cop = isnothing(coin_out) ? C_NULL : pointer(co)
        GC.@preserve idx ci co lim a o check(r.ctx,
            ccall((:cfmm_quote_to_rate, LIB), Cint,
                  (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                  r.ctx, s, length(qs), idx, ci, cop, lim, a, o))
        amount[qs] .= a
        out[qs] .= o
    end
    return amount, out
end

# swap_limit!(r, pools, coin_in, amount_in, rate_limit; coin_out) -- the Python host's `swap_limit_` (cfmm_swap_limit): swap!'s
# arguments and a limit on the marginal rate per swap (0.0: none).  Swap q tenders min(amount_in[q], amount_to_rate's answer on
# the pool as the earlier swaps left it); amount_in may be Inf where the limit is > 0.  Returns (amount_used, amount_out,
# status): LIMIT_FILLED, LIMIT_PARTIAL (the pool rests at the limit, to rounding), LIMIT_NONE or LIMIT_REFUSED.  A state
# change, as swap!: the router's trades are those of the old market.
function swap_limit!(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                     amount_in::AbstractVector{<:Real}, rate_limit::AbstractVector{<:Real}; coin_out=nothing)
    where, segs = limit_segments(r, pools, coin_in, amount_in, rate_limit, coin_out)
    n = length(pools)
    used = Vector{Float64}(undef, n)
    out = Vector{Float64}(undef, n)
    status = Vector{Int32}(undef, n)
    for s in sort(collect(keys(segs)))
        qs = segs[s]
        idx = Int64[where[pools[q]][2] for q in qs]
        ci = Int32[coin_in[q] - 1 for q in qs]
        co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
        amt = Float64[amount_in[q] for q in qs]
        lim = Float64[rate_limit[q] for q in qs]
        u = Vector{Float64}(undef, length(qs))
        o = Vector{Float64}(undef, length(qs))
        st = Vector{Int32}(undef, length(qs))
        cop = isnothing(coin_out) ? C_NULL : pointer(co)
        GC.@preserve idx ci co amt lim u o st check(r.ctx,
            ccall((:cfmm_swap_limit, LIB), Cint,
                  (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  r.ctx, s, length(qs), idx, ci, cop, amt, lim, u, o, st))
        used[qs] .= u
        out[qs] .= o
        status[qs] .= st
    end
    return used, out, status
end
