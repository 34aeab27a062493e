# quote_to_rate.jl -- the tests of amount_to_rate and swap_limit! (cfmm_quote_to_rate, cfmm_swap_limit), runnable on their own:
#     julia --project=julia julia/test/quote_to_rate.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

@testset "amount_to_rate / swap_limit!: the amount to a target rate, and the swap that stops there" begin
    pools = CFMM{Float64}[ProductTwoCoin([1.0e5, 2.0e5], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 4.0e4], 0.999, [2, 3])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    spot = spot_price(r, [1], [1])[1]
    a, out = amount_to_rate(r, [1, 1], [1, 1], [0.81 * spot, 2 * spot])
    @test isapprox(a[1], 1.0e5 * (1 / 0.9 - 1) / 0.997; rtol=1e-13)            # x'/R_in = sqrt(s/r)
    @test a[2] == 0.0 && out[2] == 0.0                                          # the spot rate is already below the limit
    @test out == quote_swaps(r, [1, 1], [1, 1], a)                              # the bits of the quote
    @test isapprox(quote_rate(r, [1], [1], a[1:1])[2][1], 0.81 * spot; rtol=1e-13)
    used, got, status = swap_limit!(r, [1, 1, 2], [1, 1, 1], [Inf, Inf, 10.0], [0.81 * spot, 0.81 * spot * (1 + 1e-9), 0.0])
    @test used[1] == a[1] && got[1] == out[1] && status[1] == CFMMRouterAMD.LIMIT_PARTIAL
    @test used[2] == 0.0 && status[2] == CFMMRouterAMD.LIMIT_NONE               # the pool rests at the limit
    @test used[3] == 10.0 && status[3] == CFMMRouterAMD.LIMIT_FILLED            # limit 0.0: swap!
    @test isapprox(spot_price(r, [1], [1])[1], 0.81 * spot; rtol=1e-13)
    @test_throws ArgumentError amount_to_rate(r, [1], [1], [0.0])
end
