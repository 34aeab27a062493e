# quote_rate.jl -- the tests of quote_rate, spot_price and quote_path_rate (cfmm_quote_rate, cfmm_quote_path_rate), runnable
# on their own:
#     julia --project=julia julia/test/quote_rate.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "quote_rate / spot_price / quote_path_rate: the marginal rate beside the quote" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 2.0e5], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 4.0e4], 0.999, [2, 3])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    a = [0.0, 10.0, 1000.0]
    out, rate = quote_rate(r, [1, 1, 1], [1, 1, 1], a)
    @test out == quote_swaps(r, [1, 1, 1], [1, 1, 1], a)                        # the bits of the quote
    @test rate[1] == spot_price(r, [1], [1])[1]                                 # the rate at 0 is the spot rate
    @test isapprox(rate[1], 0.997 * 2.0e5 / 1.0e5; rtol=1e-14)                  # γ·R_out/R_in
    @test rate[1] > rate[2] > rate[3] > 0                                       # the next unit buys less and less
    pout, prate, hv, hr = quote_path_rate(r, [[1, 2]], [[1, 2, 3]], [10.0]; hops=true)
    @test pout == quote_paths(r, [[1, 2]], [[1, 2, 3]], [10.0])
    @test hr[1, 1] == rate[2] && prate[1] == hr[1, 1] * hr[1, 2]                # the chain rule, hop by hop
    @test_throws ArgumentError quote_rate(r, [1], [1], [-1.0])
end
