# find_disjoint_paths_out.jl -- the tests of find_disjoint_paths_out (cfmm_find_disjoint_paths_out), runnable on their own:
#     julia --project=julia julia/test/find_disjoint_paths_out.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "find_disjoint_paths_out: the routes that can each give a share, then split_paths_out on them" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
                          ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
                          ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    B = 1.5e5
    cost, found, toks, st = find_disjoint_paths_out(r, [1, 1, 1], [2, 2, 2], [1.0e4, B, B / 4]; max_paths=8)
    @test Set(found[1]) == Set([[1], [2], [3], [4, 5]]) && all(st[1] .== 0)                     # every route can give 10 000
    @test issorted(cost[1]) && quote_paths_out(r, found[1], toks[1], fill(1.0e4, 4)) == cost[1] # cheapest first, bit for bit
    @test find_paths_out(r, [1], [2], [1.0e4])[2][1] == found[1][1]                             # the first is find_paths_out's
    @test isempty(found[2])                                                                     # no path gives 150 000 alone
    @test Set(found[3]) == Set([[1], [2], [4, 5]])                                              # three can carry a quarter of it
    x, c, total, status = split_paths_out(r, [found[3]], [toks[3]], [B])
    @test status == [0] && isfinite(total[1]) && abs(sum(x[1]) - B) <= 1e-15 * B
    @test_throws ArgumentError find_disjoint_paths_out(r, [1], [2], [B]; max_paths=9)
    @test_throws ArgumentError find_disjoint_paths_out(r, [1], [4], [B])
end
