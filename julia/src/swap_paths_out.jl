# swap_paths_out.jl -- part of module CFMMRouterAMD (included from CFMMRouterAMD.jl): the exact-output form of swap_paths!.
# Its entry, cfmm_swap_path_out, is declared in include/cfmm_amd_path_out.h, beside include/cfmm_amd.h.

# swap_paths_out!(r, pools, tokens, amount_out; max_in=nothing, hops=false, sync=true) -- the Python host's `swap_path_out_`
# (cfmm_swap_path_out): quote_paths_out's arguments, mapping and refusals, but the paths are EXECUTED in the order given, each
# all or nothing: "buy exactly amount_out[p] through the path, revert if it costs more than max_in[p]".  Path p sees the market
# as the applied paths before it left it; its amounts are what quote_paths_out answers on that market and each pool of an
# applied path moves as swap_out! moves it.  Returns (amount_in, status[, hop_in]) with swap_out!'s status codes.
function swap_paths_out!(r::AMDRouter, pools::AbstractVector, tokens::AbstractVector, amount_out::AbstractVector{<:Real};
                         max_in=nothing, hops::Bool=false, sync::Bool=true)
    n, H, n_hops, seg, row, ci, co, amt = path_hop_arrays(r, pools, tokens, amount_out)
    (isnothing(max_in) || length(max_in) == n) || throw(ArgumentError("max_in must have one entry per path"))
    lim = isnothing(max_in) ? Float64[] : Float64[max_in[p] for p in 1:n]
    out = Vector{Float64}(undef, n)
    status = Vector{Int32}(undef, n)
    hv = fill(NaN, n, H)
    n == 0 && return hops ? (out, status, hv) : (out, status)
    hp = hops ? pointer(hv) : Ptr{Float64}(C_NULL)
    lp = isnothing(max_in) ? Ptr{Float64}(C_NULL) : pointer(lim)
    try
        GC.@preserve n_hops seg row ci co amt lim out hv status check(r.ctx,
            ccall((:cfmm_swap_path_out, LIB), Cint,
                  (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  r.ctx, n, H, n_hops, seg, row, ci, co, amt, lp, out, hp, status))
        sync && download_state!(r)
    finally
        foreach(d -> fill!(d, 0), r.Δs); foreach(l -> fill!(l, 0), r.Λs)
    end
    return hops ? (out, status, hv) : (out, status)
end
