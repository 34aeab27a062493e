# find_disjoint_paths.jl -- the tests of find_disjoint_paths (cfmm_find_disjoint_paths), runnable on their own:
#     julia --project=julia julia/test/find_disjoint_paths.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "find_disjoint_paths: the four routes of an order found on the device, then split and executed" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
                          ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
                          ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    A = 1.0e5
    out, paths, toks, st = find_disjoint_paths(r, [1], [2], [A]; max_paths=8, max_hops=3)
    @test Set(paths[1]) == Set([[1], [2], [3], [4, 5]])                                         # every route, no pool twice
    @test all(st[1] .== 0) && issorted(out[1]; rev=true)
    @test paths[1][1] == find_paths(r, [1], [2], [A])[2][1] && out[1][1] == find_paths(r, [1], [2], [A])[1][1]
    @test quote_paths(r, paths[1], toks[1], fill(A, 4)) == out[1]                               # quoted bit for bit
    @test length(find_disjoint_paths(r, [1], [2], [A]; max_paths=2)[2][1]) == 2
    @test find_disjoint_paths(r, [1], [2], [0.0])[2][1] == []                                   # nothing to carry: nothing found
    x, y, total, sst = split_paths(r, [paths[1]], [toks[1]], [A])                               # find -> split -> execute
    @test sst == [0] && total[1] > out[1][1]
    got, status = swap_paths!(r, paths[1], toks[1], x[1])
    @test all(status .== 0) && got == y[1]
    @test_throws ArgumentError find_disjoint_paths(r, [1], [2], [A]; max_paths=9)
    @test_throws ArgumentError find_disjoint_paths(r, [9], [1], [1.0])
end
