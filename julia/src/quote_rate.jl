# quote_rate.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): marginal rates of the exact-input quotes.
# Its entries, cfmm_quote_rate and cfmm_quote_path_rate, are declared in include/cfmm_amd_rate.h, beside include/cfmm_amd.h.

# one cfmm_quote_rate call per segment that has a query; amount_in = nothing: no amounts (the spot rate), the amounts out are
# then not asked for and come back as NaN
function quote_rate_queries(r::AMDRouter, pools, coin_in, amount_in, coin_out)
    n = length(pools)
    (length(coin_in) == n && (isnothing(amount_in) || length(amount_in) == n) && (isnothing(coin_out) || length(coin_out) == n)) ||
        throw(ArgumentError("coin_in, the amounts and coin_out must have one entry per pool"))
    where = segment_rows(r)
    segs = Dict{Int32,Vector{Int}}()                      # segment => query numbers
    for (q, i) in enumerate(pools)
        i in r.host && throw(ArgumentError("pool $i: $(typeof(r.cfmms[i])) is evaluated on the host by its own find_arb! and has no device state to quote"))
        haskey(where, i) || throw(ArgumentError("pool $i out of range"))
        push!(get!(segs, where[i][1], Int[]), q)
    end
    out = fill(NaN, n)
    rate = Vector{Float64}(undef, n)
    for s in sort(collect(keys(segs)))
        qs = segs[s]
        idx = Int64[where[pools[q]][2] for q in qs]
        ci = Int32[coin_in[q] - 1 for q in qs]
        co = isnothing(coin_out) ? Int32[] : Int32[coin_out[q] - 1 for q in qs]
        amt = isnothing(amount_in) ? Float64[] : Float64[amount_in[q] for q in qs]
        res = Vector{Float64}(undef, length(qs))
        rt = Vector{Float64}(undef, length(qs))
        cop = isnothing(coin_out) ? C_NULL : pointer(co)
        ap = isnothing(amount_in) ? Ptr{Float64}(C_NULL) : pointer(amt)
        rp = isnothing(amount_in) ? Ptr{Float64}(C_NULL) : pointer(res)
        GC.@preserve idx ci co amt res rt check(r.ctx,
            ccall((:cfmm_quote_rate, LIB), Cint,
                  (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                  r.ctx, s, length(qs), idx, ci, cop, ap, rp, rt))
        isnothing(amount_in) || (out[qs] .= res)
        rate[qs] .= rt
    end
    return out, rate
end

# quote_rate(r, pools, coin_in, amount_in; coin_out) -- the Python host's router-level `quote_rate` (cfmm_quote_rate): quote_swaps'
# arguments, mapping and refusals; returns (amount_out, rate).  amount_out is quote_swaps' answer bit for bit; rate[q] is the right
# derivative of the quote at amount_in[q] -- units of the coin out per unit of the coin in for the next unit tendered, fee
# included; at amount 0 the pool's spot rate; 0.0 once a UniV3 ladder is exhausted.
function quote_rate(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer},
                    amount_in::AbstractVector{<:Real}; coin_out=nothing)
    return quote_rate_queries(r, pools, coin_in, amount_in, coin_out)
end

# spot_price(r, pools, coin_in; coin_out) -- the Python host's `spot_price`: the rate at amount 0, fee included, without
# tendering anything (cfmm_quote_rate with no amounts).
function spot_price(r::AMDRouter, pools::AbstractVector{<:Integer}, coin_in::AbstractVector{<:Integer}; coin_out=nothing)
    return quote_rate_queries(r, pools, coin_in, nothing, coin_out)[2]
end

# quote_path_rate(r, pools, tokens, amount_in; hops=false) -- the Python host's `quote_path_rate` (cfmm_quote_path_rate):
# quote_paths' arguments, mapping and refusals; returns (amount_out, rate[, hop_out, hop_rate]).  amount_out / hop_out are
# quote_paths' bit for bit, hop_rate[p, k] is quote_rate of hop k at the amount entering it and rate[p] their left-fold
# product ((r_1·r_2)·r_3)..., the path's marginal rate.  A hop through an exhausted UniV3 ladder makes the path's rate 0.0.
function quote_path_rate(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_in::AbstractVector{<:Real}; hops::Bool=false)
    n, H, n_hops, seg, row, ci, co, amt = path_hop_arrays(r, pools, tokens, amount_in)
    out = Vector{Float64}(undef, n)
    rate = Vector{Float64}(undef, n)
    hv = fill(NaN, n, H); hr = fill(NaN, n, H)
    n == 0 && return hops ? (out, rate, hv, hr) : (out, rate)
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    hrp = hops ? pointer(hr) : Ptr{Float64}(C_NULL)
    GC.@preserve n_hops seg row ci co amt out rate hv hr check(r.ctx,
        ccall((:cfmm_quote_path_rate, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}),
              r.ctx, n, H, n_hops, seg, row, ci, co, amt, out, rate, hp, hrp))
    return hops ? (out, rate, hv, hr) : (out, rate)
end
