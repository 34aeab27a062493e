# split_paths_out.jl -- the tests of split_paths_out (cfmm_split_paths_out), runnable on their own:
#     julia --project=julia julia/test/split_paths_out.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "split_paths_out: an amount no single path can give, bought through three parallel pools and a detour, then executed" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
                          ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
                          ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    paths = [[1], [2], [3], [4, 5]]
    toks = [[1, 2], [1, 2], [1, 2], [1, 3, 2]]
    B = 1.5e5
    @test all(isinf, quote_paths_out(r, paths, toks, fill(B, 4)))                               # no single path can give it
    x, c, total, st = split_paths_out(r, [paths, [[1]], [[2], [3]]], [toks, [[1, 2]], [[1, 2], [1, 2]]], [B, 123.456, 1.0e5])
    @test st == [0, 0, 4]                                                                       # SPLIT_OK, SPLIT_OK, SPLIT_UNOBTAINABLE
    @test abs(sum(x[1]) - B) <= 1e-15 * B && all(x[1] .> 0) && x[1][1] > x[1][2] > x[1][3]      # deeper pools give more
    @test x[2] == [123.456]                                                                     # one path: the amount, bit for bit
    @test quote_paths_out(r, paths, toks, x[1]) == c[1]                                         # the round trip, bit for bit
    @test total[1] == ((c[1][1] + c[1][2]) + c[1][3]) + c[1][4] && isfinite(total[1])
    @test total[3] == Inf && all(c[3] .== Inf) && all(x[3] .== 0.0)                             # more than the two pools hold
    @test split_paths_out(r, [paths], [toks], [0.0])[4] == [1]                                  # nothing to buy: SPLIT_NONE
    paid, status = swap_paths_out!(r, paths, toks, x[1]; max_in=c[1])                           # one call executes the split
    @test all(status .== 0) && paid == c[1]
    @test_throws ArgumentError split_paths_out(r, [paths], [toks], [B]; rounds=17)
    @test_throws ArgumentError split_paths_out(r, [[[1], [2], [1]]], [[[1, 2], [1, 2], [1, 2]]], [B])   # a pool twice in an order
    @test_throws ArgumentError split_paths_out(r, [fill([1], 9)], [fill([1, 2], 9)], [B])               # nine paths
end
