# find_disjoint_paths.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): several swap paths per order that
# share no pool, found on the device.  Its entry, cfmm_find_disjoint_paths, is declared in include/cfmm_amd_find_disjoint.h,
# beside include/cfmm_amd.h.

# find_disjoint_paths(r, token_in, token_out, amount_in; max_paths=4, max_hops=3, usable_only=true) -- the Python host's
# router-level `find_disjoint_paths` (cfmm_find_disjoint_paths): for every query up to max_paths (1 .. 8) paths from token_in[q]
# to token_out[q] (token ids as in Ai) of at most max_hops (1 .. 8) pools such that NO POOL OCCURS IN TWO OF THEM, found on the
# device among the pools as they stand there.  Returns (amount_out, pools, tokens, status): pools[q] / tokens[q] are VECTORS OF
# PATHS, exactly the pools[g] / tokens[g] split_paths takes; amount_out[q] and status[q] have one entry per listed path.  The
# contract is successive search: path k is find_paths' answer for amount_in[q] on the market without every pool of the query's
# paths before it -- greedy successive-best, not "the K best overall".  The first path is find_paths', the amounts do not
# increase along the list, and quote_paths at amount_in[q] answers each bit for bit.  The same amount probes every round: to
# split A over K paths, A / K may be the better probe.  usable_only=true leaves out the paths of status 2 (FOUND_REPEATS: a walk
# that visits a pool twice, which split_paths would refuse; its pools stay banned for the paths after it).  Host-evaluated
# pools are not searched.  Read-only.
function find_disjoint_paths(r::AMDRouter, token_in::AbstractVector{<:Integer}, token_out::AbstractVector{<:Integer},
                             amount_in::AbstractVector{<:Real}; max_paths::Integer=4, max_hops::Integer=3, usable_only::Bool=true)
    n = length(token_in)
    (length(token_out) == n && length(amount_in) == n) || throw(ArgumentError("token_in, token_out and amount_in must have one entry per query"))
    nt = length(r.v)
    for q in 1:n
        1 <= token_in[q] <= nt || throw(ArgumentError("query $q: token_in $(token_in[q]) out of range 1:$nt"))
        1 <= token_out[q] <= nt || throw(ArgumentError("query $q: token_out $(token_out[q]) out of range 1:$nt"))
    end
    1 <= max_paths <= MAX_SPLIT_PATHS || throw(ArgumentError("max_paths must be 1 to $MAX_SPLIT_PATHS"))
    1 <= max_hops <= MAX_PATH_HOPS || throw(ArgumentError("max_hops must be 1 to $MAX_PATH_HOPS"))
    K = Int(max_paths); H = Int(max_hops)
    tin = Int32[token_in[q] - 1 for q in 1:n]; tout = Int32[token_out[q] - 1 for q in 1:n]       # 0-based for the library
    amt = Float64[amount_in[q] for q in 1:n]
    n_paths = Vector{Int32}(undef, n)
    out = Matrix{Float64}(undef, n, K); n_hops = Matrix{Int32}(undef, n, K); status = Matrix{Int32}(undef, n, K)
    seg = fill(Int32(-1), n, H, K); ci = fill(Int32(-1), n, H, K); co = fill(Int32(-1), n, H, K)  # column-major [count, max_hops, max_paths] IS
    row = fill(Int64(-1), n, H, K)                                                               # the library's [max_paths][max_hops][count]
    amounts = Vector{Vector{Float64}}(undef, n); statuses = Vector{Vector{Int32}}(undef, n)
    pools = Vector{Vector{Vector{Int}}}(undef, n); tokens = Vector{Vector{Vector{Int}}}(undef, n)
    n == 0 && return amounts, pools, tokens, statuses
    GC.@preserve tin tout amt n_paths out n_hops status seg row ci co check(r.ctx,
        ccall((:cfmm_find_disjoint_paths, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
               Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}),
              r.ctx, n, K, H, tin, tout, amt, n_paths, out, n_hops, status, seg, row, ci, co))
    pool_at = Dict{Tuple{Int32,Int64},Int}(sr => i for (i, sr) in segment_rows(r))
    for q in 1:n
        keep = [k for k in 1:n_paths[q] if !(usable_only && status[q, k] == FOUND_REPEATS)]
        pools[q] = [Int[pool_at[(seg[q, h, k], row[q, h, k])] for h in 1:n_hops[q, k]] for k in keep]
        tokens[q] = [vcat(Int(token_in[q]), Int[r.cfmms[pools[q][j][h]].Ai[co[q, h, k] + 1] for h in 1:n_hops[q, k]]) for (j, k) in enumerate(keep)]
        amounts[q] = out[q, keep]; statuses[q] = status[q, keep]
    end
    return amounts, pools, tokens, statuses
end
