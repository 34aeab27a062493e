# find_disjoint_paths_out.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl, behind find_disjoint_paths.jl):
# several swap paths per order that share no pool, found on the device FOR A WANTED OUTPUT.  Its entry,
# cfmm_find_disjoint_paths_out, is declared in include/cfmm_amd_find_disjoint_out.h.

# find_disjoint_paths_out(r, token_in, token_out, amount_out; max_paths=4, max_hops=3, usable_only=true) -- the Python host's
# router-level `find_disjoint_paths_out` (cfmm_find_disjoint_paths_out): find_disjoint_paths with the direction turned.  Returns
# (amount_in, pools, tokens, status): pools[q] / tokens[q] are VECTORS OF PATHS, exactly what split_paths_out takes;
# amount_in[q] is what each listed path asks for amount_out[q].  Path k is find_paths_out's answer on the market without every
# pool of the query's paths before it: the first path is find_paths_out's, the amounts do not decrease along the list, and
# quote_paths_out at amount_out[q] answers each bit for bit.  The same amount probes every round, and A PATH THAT CANNOT GIVE IT
# ALONE IS NEVER FOUND: to buy B through K paths probe with about B / K.  usable_only as in find_disjoint_paths.  Read-only.
function find_disjoint_paths_out(r::AMDRouter, token_in::AbstractVector{<:Integer}, token_out::AbstractVector{<:Integer},
                                 amount_out::AbstractVector{<:Real}; max_paths::Integer=4, max_hops::Integer=3, usable_only::Bool=true)
    n = length(token_in)
    (length(token_out) == n && length(amount_out) == n) || throw(ArgumentError("token_in, token_out and amount_out must have one entry per query"))
    nt = length(r.v)
    for q in 1:n
        1 <= token_in[q] <= nt || throw(ArgumentError("query $q: token_in $(token_in[q]) out of range 1:$nt"))
        1 <= token_out[q] <= nt || throw(ArgumentError("query $q: token_out $(token_out[q]) out of range 1:$nt"))
    end
    1 <= max_paths <= MAX_SPLIT_PATHS || throw(ArgumentError("max_paths must be 1 to $MAX_SPLIT_PATHS"))
    1 <= max_hops <= MAX_PATH_HOPS || throw(ArgumentError("max_hops must be 1 to $MAX_PATH_HOPS"))
    K = Int(max_paths); H = Int(max_hops)
    tin = Int32[token_in[q] - 1 for q in 1:n]; tout = Int32[token_out[q] - 1 for q in 1:n]       # 0-based for the library
    amt = Float64[amount_out[q] for q in 1:n]
    n_paths = Vector{Int32}(undef, n)
    out = Matrix{Float64}(undef, n, K); n_hops = Matrix{Int32}(undef, n, K); status = Matrix{Int32}(undef, n, K)
    seg = fill(Int32(-1), n, H, K); ci = fill(Int32(-1), n, H, K); co = fill(Int32(-1), n, H, K)  # column-major [count, max_hops, max_paths] IS
    row = fill(Int64(-1), n, H, K)                                                               # the library's [max_paths][max_hops][count]
    amounts = Vector{Vector{Float64}}(undef, n); statuses = Vector{Vector{Int32}}(undef, n)
    pools = Vector{Vector{Vector{Int}}}(undef, n); tokens = Vector{Vector{Vector{Int}}}(undef, n)
    n == 0 && return amounts, pools, tokens, statuses
    GC.@preserve tin tout amt n_paths out n_hops status seg row ci co check(r.ctx,
        ccall((:cfmm_find_disjoint_paths_out, LIB), Cint,
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
