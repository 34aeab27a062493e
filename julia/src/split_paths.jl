# split_paths.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): splitting an order over several swap paths on
# the device.  Its entry, cfmm_split_paths, is declared in include/cfmm_amd_split.h, beside include/cfmm_amd.h.

const SPLIT_OK, SPLIT_NONE, SPLIT_NAN, SPLIT_SATURATED = Int32(0), Int32(1), Int32(2), Int32(3)   # CFMM_SPLIT_*
const MAX_SPLIT_PATHS = 8     # CFMM_MAX_SPLIT_PATHS
const MAX_SPLIT_ROUNDS = 16   # CFMM_MAX_SPLIT_ROUNDS

# split_paths(r, pools, tokens, amount_in; rounds=5) -- the Python host's router-level `split_paths` (cfmm_split_paths): HOW
# MUCH OF AN ORDER GOES DOWN EACH PATH, on the pools as they stand on the device.  pools[g] is a vector of 1 .. 8 paths, each a
# vector of positions in r.cfmms; tokens[g][k] the token ids along path k (1-based as in Ai, one more than the pools);
# amount_in[g] the amount of order g.  The mapping and refusals are quote_paths' (a path is named by its number in the whole
# call), and two more: every path of an order must start at the same token and end at the same token, and no pool may occur
# twice in an order -- the paths are quoted independently against the standing market, so a shared pool would be counted twice.
# Returns (path_amount_in, path_amount_out, total_out, status): the first two shaped like pools (one vector per order), the
# last two with one entry per order.  The contract is the greedy search with scaling of include/cfmm_amd_split.h: `rounds`
# (1 .. 16) rounds of 64 grid points per path; a round hands out 63 slices of what is left, each to the path whose next slice
# buys the most, then steps every share back one slice and refines.  The shares sum to the amount; quote_paths at a share
# answers its output bit for bit.  status[g] is SPLIT_OK, SPLIT_SATURATED (part of the amount buys nothing: the paths cannot
# absorb it), SPLIT_NONE (amount 0, or nothing comes out: zeros) or SPLIT_NAN.
# swap_paths!(r, pools[g], tokens[g], path_amount_in[g]) executes order g's split.  Read-only.
function split_paths(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_in::AbstractVector{<:Real}; rounds::Integer=5)
    G = length(pools)
    (length(tokens) == G && length(amount_in) == G) || throw(ArgumentError("tokens and amount_in must have one entry per order"))
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
    amt = Float64[amount_in[g] for g in 1:G]
    x = Vector{Float64}(undef, n); y = Vector{Float64}(undef, n); total = Vector{Float64}(undef, G)
    status = Vector{Int32}(undef, G)
    cut(v) = [v[first[g]+1:first[g+1]] for g in 1:G]
    G == 0 && return cut(x), cut(y), total, status
    GC.@preserve first amt n_hops seg row ci co x y total status check(r.ctx,
        ccall((:cfmm_split_paths, LIB), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32,
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
              r.ctx, G, first, amt, n, H, n_hops, seg, row, ci, co, rounds, x, y, total, status))
    return cut(x), cut(y), total, status
end
