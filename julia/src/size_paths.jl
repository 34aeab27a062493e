# size_paths.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): sizing swap paths on the device.
# Its entry, cfmm_size_path, is declared in include/cfmm_amd_size_path.h, beside include/cfmm_amd.h.

const SIZED, SIZED_NONE, SIZED_AT_LIMIT, SIZED_NAN = Int32(0), Int32(1), Int32(2), Int32(3)   # CFMM_SIZED*
const MAX_SIZE_ROUNDS = 16   # CFMM_MAX_SIZE_ROUNDS

# size_paths(r, pools, tokens, max_in; value_in=nothing, value_out=nothing, rounds=5) -- the Python host's router-level
# `size_path` (cfmm_size_path): HOW MUCH to put into each path, on the pools as they stand on the device.  pools[p] / tokens[p]
# are quote_paths' (positions in r.cfmms; the token ids along the path, 1-based as in Ai, one more than the pools), with its
# mapping and refusals; max_in[p] is the largest input to consider.  Returns (amount_in, amount_out, gain, status): the input of
# each path that maximises gain(x) = value_out[p] * quote_paths(x) - value_in[p] * x (nothing = 1.0: "out minus in", the profit
# of a cycle), what quote_paths answers for it bit for bit, and that gain.  The contract is the bracketing search: `rounds`
# (1 .. 16) rounds of 64 trial sizes spread evenly over a bracket that starts as [0, max_in] and becomes the two neighbours of
# the best trial size; a path's gain is concave, so the bracket shrinks by 2/63 per round around the maximiser.  status[p] is
# SIZED, SIZED_AT_LIMIT (gain > 0 at amount_in == max_in: the limit binds), SIZED_NONE (no size gains: three 0.0) or SIZED_NAN.
# It sizes ONE path on the STANDING market.  swap_paths!(r, pools, tokens, amount_in; min_out=...) executes the answer.  Read-only.
function size_paths(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, max_in::AbstractVector{<:Real};
                    value_in::Union{Nothing,AbstractVector{<:Real}}=nothing, value_out::Union{Nothing,AbstractVector{<:Real}}=nothing,
                    rounds::Integer=5)
    n, H, n_hops, seg, row, ci, co, lim = path_hop_arrays(r, pools, tokens, max_in)
    1 <= rounds <= MAX_SIZE_ROUNDS || throw(ArgumentError("rounds must be 1 to $MAX_SIZE_ROUNDS"))
    for (name, v) in (("value_in", value_in), ("value_out", value_out))
        (isnothing(v) || length(v) == n) || throw(ArgumentError("$name must have one entry per path"))
    end
    vi = isnothing(value_in) ? Float64[] : Float64[value_in[p] for p in 1:n]
    vo = isnothing(value_out) ? Float64[] : Float64[value_out[p] for p in 1:n]
    amount_in = Vector{Float64}(undef, n); amount_out = Vector{Float64}(undef, n); gain = Vector{Float64}(undef, n)
    status = Vector{Int32}(undef, n)
    n == 0 && return amount_in, amount_out, gain, status
    vip = isnothing(value_in) ? Ptr{Float64}(C_NULL) : pointer(vi)
    vop = isnothing(value_out) ? Ptr{Float64}(C_NULL) : pointer(vo)
    GC.@preserve n_hops seg row ci co lim vi vo amount_in amount_out gain status check(r.ctx,
        ccall((:cfmm_size_path, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
              r.ctx, n, H, n_hops, seg, row, ci, co, lim, vip, vop, rounds, amount_in, amount_out, gain, status))
    return amount_in, amount_out, gain, status
end
