# find_paths_out.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): the exact-output form of find_paths.
# Its entry, cfmm_find_path_out, is declared in include/cfmm_amd_find_out.h, beside include/cfmm_amd.h.

# find_paths_out(r, token_in, token_out, amount_out; max_hops=3) -- the Python host's router-level `find_path_out`
# (cfmm_find_path_out): the CHEAPEST swap path of at most max_hops (1 .. 8) pools that buys exactly amount_out[q] of
# token_out[q], paid in token_in[q] (token ids as in Ai), FOUND on the device among the pools as they stand there.  Returns
# (amount_in, pools, tokens, status): pools[q] / tokens[q] in the form quote_paths_out / swap_paths_out! take (positions in
# r.cfmms; the tokens along the path from token_in to token_out, one more than the pools), empty where nothing was found.  The
# contract is find_paths' layered search run backwards from the wanted output: layer h holds per token the smallest quote_out
# over every pool and ordered coin pair into layer h-1, every hop quoted against the pool as it stands; the answer is the
# smallest layer entry of token_in with the fewest hops, walked forward with ties to the smallest (segment, row, coin_in,
# coin_out) -- quote_paths_out on the result answers amount_in bit for bit.  status[q] is FOUND, FOUND_REPEATS (the walk visits
# a pool twice: swap_paths_out! refuses it as one path) or FOUND_NONE with amount_in Inf (token_in not reached within max_hops:
# no pool can give that much) or 0.0 (amount_out 0: nothing to buy).  Host-evaluated pools are not searched.  Read-only.
function find_paths_out(r::AMDRouter, token_in::AbstractVector{<:Integer}, token_out::AbstractVector{<:Integer},
                        amount_out::AbstractVector{<:Real}; max_hops::Integer=3)
    n = length(token_in)
    (length(token_out) == n && length(amount_out) == n) || throw(ArgumentError("token_in, token_out and amount_out must have one entry per query"))
    nt = length(r.v)
    for q in 1:n
        1 <= token_in[q] <= nt || throw(ArgumentError("query $q: token_in $(token_in[q]) out of range 1:$nt"))
        1 <= token_out[q] <= nt || throw(ArgumentError("query $q: token_out $(token_out[q]) out of range 1:$nt"))
    end
    1 <= max_hops <= MAX_PATH_HOPS || throw(ArgumentError("max_hops must be 1 to $MAX_PATH_HOPS"))
    H = Int(max_hops)
    tin = Int32[token_in[q] - 1 for q in 1:n]; tout = Int32[token_out[q] - 1 for q in 1:n]       # 0-based for the library
    amt = Float64[amount_out[q] for q in 1:n]
    cost = Vector{Float64}(undef, n)
    n_hops = Vector{Int32}(undef, n); status = Vector{Int32}(undef, n)
    seg = fill(Int32(-1), n, H); ci = fill(Int32(-1), n, H); co = fill(Int32(-1), n, H)          # column-major [count, max_hops] IS the
    row = fill(Int64(-1), n, H)                                                                  # library's hop-major layout
    n == 0 && return cost, Vector{Int}[], Vector{Int}[], status
    GC.@preserve tin tout amt cost n_hops seg row ci co status check(r.ctx,
        ccall((:cfmm_find_path_out, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
              r.ctx, n, H, tin, tout, amt, cost, n_hops, seg, row, ci, co, status))
    pool_at = Dict{Tuple{Int32,Int64},Int}(sr => i for (i, sr) in segment_rows(r))
    pools = Vector{Vector{Int}}(undef, n); tokens = Vector{Vector{Int}}(undef, n)
    for q in 1:n
        pools[q] = Int[pool_at[(seg[q, k], row[q, k])] for k in 1:n_hops[q]]
        tokens[q] = n_hops[q] == 0 ? Int[] : vcat(Int(token_in[q]), Int[r.cfmms[pools[q][k]].Ai[co[q, k] + 1] for k in 1:n_hops[q]])
    end
    return cost, pools, tokens, status
end
