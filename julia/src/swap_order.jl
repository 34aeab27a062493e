# swap_order.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl, behind split_paths_out.jl): executing split
# orders on the device, each order all or nothing ACROSS its paths, in both directions.  The entries, cfmm_swap_order and
# cfmm_swap_order_out, are declared in include/cfmm_amd_order.h.

const ORDER_APPLIED = Int32(0)        # CFMM_ORDER_APPLIED
const ORDER_LIMIT = Int32(1)          # CFMM_ORDER_LIMIT
const ORDER_REFUSED = Int32(2)        # CFMM_ORDER_REFUSED
const ORDER_UNOBTAINABLE = Int32(3)   # CFMM_ORDER_UNOBTAINABLE (swap_orders_out! only)
const ORDER_PATH_HELD = Int32(4)      # CFMM_ORDER_PATH_HELD: a path that passes in an order that was not applied

# what both verbs do before the library is called: split_paths' shaping and refusals of the orders, path_hop_arrays' of the
# flat paths.  path_amount: one vector per order, shaped like pools.  Returns (G, first, n, H, n_hops, seg, row, ci, co, amt).
function order_hop_arrays(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, path_amount::AbstractVector)
    G = length(pools)
    (length(tokens) == G && length(path_amount) == G) || throw(ArgumentError("tokens and the path amounts must have one entry per order"))
    first = zeros(Int64, G + 1)                                                      # 0-based for the library
    for g in 1:G
        1 <= length(pools[g]) <= MAX_SPLIT_PATHS || throw(ArgumentError("order $g: $(length(pools[g])) paths (an order has 1 to $MAX_SPLIT_PATHS)"))
        length(tokens[g]) == length(pools[g]) || throw(ArgumentError("order $g: $(length(tokens[g])) token sequences for $(length(pools[g])) paths"))
        length(path_amount[g]) == length(pools[g]) || throw(ArgumentError("order $g: $(length(path_amount[g])) amounts for $(length(pools[g])) paths"))
        first[g+1] = first[g] + length(pools[g])
    end
    flat_pools = [p for o in pools for p in o]
    flat_tokens = [t for o in tokens for t in o]
    flat_amount = Float64[a for o in path_amount for a in o]
    n, H, n_hops, seg, row, ci, co, amt = path_hop_arrays(r, flat_pools, flat_tokens, flat_amount)
    for g in 1:G
        ends = unique([(t[1], t[end]) for t in tokens[g]])
        length(ends) == 1 || throw(ArgumentError("order $g: its paths must all start at the same token and end at the same token"))
        seen = Dict{Int,Int}()
        for (k, path) in enumerate(pools[g]), i in path
            haskey(seen, i) && throw(ArgumentError("order $g: paths $(seen[i]) and $k share pool $i (the paths are walked against one market)"))
            seen[i] = k
        end
    end
    return G, first, n, H, n_hops, seg, row, ci, co, amt
end

# swap_orders!(r, pools, tokens, path_amount_in; min_total_out=nothing, hops=false, sync=true) -- the Python host's `swap_order_`
# (cfmm_swap_order): pools[g] / tokens[g] are lists of paths exactly as split_paths takes and answers them, path_amount_in[g] the
# amount going down each path of order g.  The orders are EXECUTED in the order given, each ALL OR NOTHING ACROSS ITS PATHS: every
# path is walked as swap_paths! walks it on the market the applied orders before left, the outputs are added in path order, and
# only when no path refuses and the total clears min_total_out[g] does any pool move.  Returns (path_amount_out, total_out, status,
# path_status[, hop_out]); the first and path_status shaped like pools; status[g] is ORDER_APPLIED, ORDER_LIMIT or ORDER_REFUSED,
# path_status 0 (applied), 2 (this path refuses) or ORDER_PATH_HELD.
function swap_orders!(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, path_amount_in::AbstractVector;
                      min_total_out=nothing, hops::Bool=false, sync::Bool=true)
    G, first, n, H, n_hops, seg, row, ci, co, amt = order_hop_arrays(r, pools, tokens, path_amount_in)
    (isnothing(min_total_out) || length(min_total_out) == G) || throw(ArgumentError("min_total_out must have one entry per order"))
    lim = isnothing(min_total_out) ? Float64[] : Float64[min_total_out[g] for g in 1:G]
    out = Vector{Float64}(undef, n); total = Vector{Float64}(undef, G)
    status = Vector{Int32}(undef, G); path_status = Vector{Int32}(undef, n)
    hv = fill(NaN, n, H)
    cut(v) = [v[first[g]+1:first[g+1]] for g in 1:G]
    G == 0 && return hops ? (cut(out), total, status, cut(path_status), hv) : (cut(out), total, status, cut(path_status))
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    lp = isnothing(min_total_out) ? Ptr{Float64}(C_NULL) : pointer(lim)
    try
        GC.@preserve first n_hops seg row ci co amt lim out hv total path_status status check(r.ctx,
            ccall((:cfmm_swap_order, LIB), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                  r.ctx, G, first, n, H, n_hops, seg, row, ci, co, amt, lp, out, hp, total, path_status, status))
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return hops ? (cut(out), total, status, cut(path_status), hv) : (cut(out), total, status, cut(path_status))
end

# swap_orders_out!(r, pools, tokens, path_amount_out; max_total_in=nothing, hops=false, sync=true) -- the Python host's
# `swap_order_out_` (cfmm_swap_order_out), the exact-output twin: path_amount_out[g] is what each path of order g is to give, as
# split_paths_out answers it; every path is walked as swap_paths_out! walks it.  Returns (path_amount_in, total_in, status,
# path_status[, hop_in]); status[g] may also be ORDER_UNOBTAINABLE (some path cannot give its amount: total Inf, that path's
# path_status 3), and ORDER_LIMIT is total_in[g] > max_total_in[g].
function swap_orders_out!(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, path_amount_out::AbstractVector;
                          max_total_in=nothing, hops::Bool=false, sync::Bool=true)
    G, first, n, H, n_hops, seg, row, ci, co, amt = order_hop_arrays(r, pools, tokens, path_amount_out)
    (isnothing(max_total_in) || length(max_total_in) == G) || throw(ArgumentError("max_total_in must have one entry per order"))
    lim = isnothing(max_total_in) ? Float64[] : Float64[max_total_in[g] for g in 1:G]
    cost = Vector{Float64}(undef, n); total = Vector{Float64}(undef, G)
    status = Vector{Int32}(undef, G); path_status = Vector{Int32}(undef, n)
    hv = fill(NaN, n, H)
    cut(v) = [v[first[g]+1:first[g+1]] for g in 1:G]
    G == 0 && return hops ? (cut(cost), total, status, cut(path_status), hv) : (cut(cost), total, status, cut(path_status))
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    lp = isnothing(max_total_in) ? Ptr{Float64}(C_NULL) : pointer(lim)
    try
        GC.@preserve first n_hops seg row ci co amt lim cost hv total path_status status check(r.ctx,
            ccall((:cfmm_swap_order_out, LIB), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                  r.ctx, G, first, n, H, n_hops, seg, row, ci, co, amt, lp, cost, hp, total, path_status, status))
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return hops ? (cut(cost), total, status, cut(path_status), hv) : (cut(cost), total, status, cut(path_status))
end
