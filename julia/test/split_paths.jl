# split_paths.jl -- the tests of split_paths (cfmm_split_paths), runnable on their own:
#     julia --project=julia julia/test/split_paths.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "split_paths: an order spread over three parallel pools and a detour, then executed" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
                          ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
                          ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    paths = [[1], [2], [3], [4, 5]]
    toks = [[1, 2], [1, 2], [1, 2], [1, 3, 2]]
    A = 1.0e5
    x, y, total, st = split_paths(r, [paths, [[1]]], [toks, [[1, 2]]], [A, 123.456])
    @test st == [0, 0]
    @test abs(sum(x[1]) - A) <= 1e-15 * A && all(x[1] .> 0) && x[1][1] > x[1][2] > x[1][3]      # deeper pools take more
    @test x[2] == [123.456]                                                                     # one path: the amount, bit for bit
    @test quote_paths(r, paths, toks, x[1]) == y[1]                                             # the round trip, bit for bit
    @test total[1] == ((y[1][1] + y[1][2]) + y[1][3]) + y[1][4]
    single = maximum(quote_paths(r, paths, toks, fill(A, 4)))
    @test total[1] > single                                                                     # better than any one path
    @test split_paths(r, [paths], [toks], [0.0])[4] == [1]                                      # nothing to spread: SPLIT_NONE
    out, status = swap_paths!(r, paths, toks, x[1])                                             # one call executes the split
    @test all(status .== 0) && out == y[1]
    @test split_paths(r, [paths], [toks], [A])[3][1] < total[1]                                 # the market it left is worse
    @test_throws ArgumentError split_paths(r, [paths], [toks], [A]; rounds=17)
    @test_throws ArgumentError split_paths(r, [[[1], [2], [1]]], [[[1, 2], [1, 2], [1, 2]]], [A])     # a pool twice in an order
    @test_throws ArgumentError split_paths(r, [[[1], [4]]], [[[1, 2], [1, 3]]], [A])                  # two different ends
    @test_throws ArgumentError split_paths(r, [fill([1], 9)], [fill([1, 2], 9)], [A])                 # nine paths
end
