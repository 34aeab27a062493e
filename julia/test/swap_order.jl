# swap_order.jl -- the tests of swap_orders! and swap_orders_out! (cfmm_swap_order, cfmm_swap_order_out), runnable on their own:
#     julia --project=julia julia/test/swap_order.jl
# They need an MI355X and the built library, like runtests.jl.
using CFMMRouter
using CFMMRouterAMD
using Test

market() = CFMM{Float64}[ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
                         ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
                         ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]

@testset "swap_orders!: a split order executed all or nothing across its paths, with one limit on its total" begin
    r = AMDRouter(LinearNonnegative(ones(3)), market(), 3)
    twin = AMDRouter(LinearNonnegative(ones(3)), market(), 3)
    paths = [[1], [2], [3], [4, 5]]
    toks = [[1, 2], [1, 2], [1, 2], [1, 3, 2]]
    x, y, total, st = split_paths(r, [paths], [toks], [1.0e5])
    @test st == [0]
    # one ulp above the split's total: held, every path ORDER_PATH_HELD, nothing moved
    out, tot, status, pst = swap_orders!(r, [paths], [toks], x; min_total_out=[nextfloat(total[1])])
    @test status == [CFMMRouterAMD.ORDER_LIMIT] && pst[1] == fill(CFMMRouterAMD.ORDER_PATH_HELD, 4) && tot == total && out[1] == y[1]
    @test all(p.R == q.R for (p, q) in zip(r.cfmms, twin.cfmms))
    # the split's own total: applied, bit for bit, and the pools stand where swap_paths! leaves the twin's
    out, tot, status, pst = swap_orders!(r, [paths], [toks], x; min_total_out=total)
    @test status == [CFMMRouterAMD.ORDER_APPLIED] && all(pst[1] .== 0) && tot == total && out[1] == y[1]
    want, want_st = swap_paths!(twin, paths, toks, x[1])
    @test all(want_st .== 0) && want == out[1]
    @test all(p.R == q.R for (p, q) in zip(r.cfmms, twin.cfmms))
    @test_throws ArgumentError swap_orders!(r, [[[1], [2], [1]]], [[[1, 2], [1, 2], [1, 2]]], [[1.0, 1.0, 1.0]])   # a pool twice in an order
    @test_throws ArgumentError swap_orders!(r, [paths], [toks], [[1.0, 2.0]])                                        # two amounts for four paths
end

@testset "swap_orders_out!: an amount no single path can give, bought through the split and executed as one order" begin
    r = AMDRouter(LinearNonnegative(ones(3)), market(), 3)
    twin = AMDRouter(LinearNonnegative(ones(3)), market(), 3)
    paths = [[1], [2], [4, 5]]
    toks = [[1, 2], [1, 2], [1, 3, 2]]
    B = 1.5e5
    @test all(isinf, quote_paths_out(r, paths, toks, fill(B, 3)))
    x, c, total, st = split_paths_out(r, [paths], [toks], [B])
    @test st == [0]
    cost, tot, status, pst = swap_orders_out!(r, [paths], [toks], x; max_total_in=[prevfloat(total[1])])
    @test status == [CFMMRouterAMD.ORDER_LIMIT] && pst[1] == fill(CFMMRouterAMD.ORDER_PATH_HELD, 3) && tot == total
    cost, tot, status, pst = swap_orders_out!(r, [paths], [toks], x; max_total_in=total)
    @test status == [CFMMRouterAMD.ORDER_APPLIED] && cost[1] == c[1] && tot == total
    paid, paid_st = swap_paths_out!(twin, paths, toks, x[1]; max_in=c[1])
    @test all(paid_st .== 0) && paid == cost[1]
    @test all(p.R == q.R for (p, q) in zip(r.cfmms, twin.cfmms))
    # a path that cannot give its share makes the whole order unobtainable: nothing moves
    cost, tot, status, pst = swap_orders_out!(twin, [[[1], [3]]], [[[1, 2], [1, 2]]], [[10.0, 1.0e6]])
    @test status == [CFMMRouterAMD.ORDER_UNOBTAINABLE] && tot == [Inf] && pst[1] == [CFMMRouterAMD.ORDER_PATH_HELD, 3]
end
