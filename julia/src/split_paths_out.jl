# split_paths_out.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl, behind split_paths.jl): buying an exact
# amount through several swap paths on the device.  Its entry, cfmm_split_paths_out, is declared in
# include/cfmm_amd_split_out.h, beside include/cfmm_amd_split.h.

const SPLIT_UNOBTAINABLE = Int32(4)   # CFMM_SPLIT_UNOBTAINABLE

# split_paths_out(r, pools, tokens, amount_out; rounds=5) -- the Python host's router-level `split_paths_out`
# (cfmm_split_paths_out): HOW MUCH OF A WANTED AMOUNT COMES OUT OF EACH PATH, on the pools as they stand on the device.  pools,
# tokens, the mapping and every refusal are split_paths'; amount_out[g] is the amount of the paths' common last token that
# order g buys.  Returns (path_amount_out, path_amount_in, total_in, status): the first two shaped like pools (the share of
# amount_out[g] bought through each path, and what quote_paths_out answers for it bit for bit), the last two with one entry per
# order.  The contract is split_paths' greedy search laid over the output (include/cfmm_amd_split_out.h): a round hands out 63
# slices of what is left, each to the path whose next slice COSTS the least (+Inf where a path cannot give that much), then
# steps every share back one slice and refines.  status[g] is SPLIT_OK; SPLIT_UNOBTAINABLE (a step found no path that can give
# another slice: costs and total Inf, shares 0.0 -- the search's verdict on its grid: paths that jointly give less than
# amount_out * (1 + K/63) may be refused though a finer split exists); SPLIT_NONE (amount 0: zeros) or SPLIT_NAN.
# swap_paths_out!(r, pools[g], tokens[g], path_amount_out[g]; max_in=path_amount_in[g]) executes order g's split.  Read-only.
function split_paths_out(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_out::AbstractVector{<:Real}; rounds::Integer=5)
    G = length(pools)
    (length(tokens) == G && length(amount_out) == G) || throw(ArgumentError("tokens and amount_out must have one entry per order"))
    1 <= rounds <= MAX_SPLIT_ROUNDS || throw(ArgumentError("rounds must be 1 to $MAX_SPLIT_ROUNDS"))
    first = zeros(Int64, G + 1)                                                      # 0-based for the library
    for g in 1:G
        1 <= length(pools[g]) <= MAX_SPLIT_PATHS || throw(ArgumentError("order $g: $(length(pools[g])) paths (an order has 1 to $MAX_SPLIT_PATHS)"))
        length(tokens[g]) == length(pools[g]) || throw(ArgumentError("order $g: $(length(tokens[g])) token sequences for $(length(pools[g])) paths"))
        first[g+1] = first[g] + length(pools[g])
    end
    flat_pools = [p for o in pools for p in o]
    flat_tokens = [t for o in tokens for t in o]
    n, H, n_hops, seg, row, ci, co, _ = path_hop_arrays(r, flat_pools, flat_tokens, zeros(length(flat_pools)))
    for g in 1:G
        ends = unique([(t[1], t[end]) for t in tokens[g]])
        length(ends) == 1 || throw(ArgumentError("order $g: its paths must all start at the same token and end at the same token"))
        seen = Dict{Int,Int}()
        for (k, path) in enumerate(pools[g]), i in path
            haskey(seen, i) && throw(ArgumentError("order $g: paths $(seen[i]) and $k share pool $i (the paths are quoted independently against the standing market)"))
            seen[i] = k
        end
    end
    amt = Float64[amount_out[g] for g in 1:G]
    x = Vector{Float64}(undef, n); y = Vector{Float64}(undef, n); total = Vector{Float64}(undef, G)
    status = Vector{Int32}(undef, G)
    cut(v) = [v[first[g]+1:first[g+1]] for g in 1:G]
    G == 0 && return cut(x), cut(y), total, status
    GC.@preserve first amt n_hops seg row ci co x y total status check(r.ctx,
        ccall((:cfmm_split_paths_out, LIB), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32,
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
              r.ctx, G, first, amt, n, H, n_hops, seg, row, ci, co, rounds, x, y, total, status))
    return cut(x), cut(y), total, status
end
