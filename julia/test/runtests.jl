# runtests.jl -- the reference's own router / CFMM tests, driven through AMDRouter on an MI355X, plus the check this
# repository cannot make anywhere else: the DEVICE against the REFERENCE ITSELF (CFMMRouter.jl's find_arb! / route! running in
# the same Julia process), pool by pool and bit for bit.
#
#     CFMM_AMD_LIB=$PWD/cfmmrouter.jl_amd/libcfmm_amd.so julia --project=julia -e 'using Pkg; Pkg.test()'
#
# STATUS: never executed (no Julia toolchain in the build image).  tests/test_julia_binding_static.py parses this file and
# checks that every AMDRouter verb it calls exists in src/CFMMRouterAMD.jl; the same scenarios run in Python against the C
# restatement of the reference (tests/test_host_cpu.py, tests/test_gpu_parity.py, tests/test_oracle_kat.py).
#
# What mirrors what (paths relative to the reference root):
#   "device sweep vs CFMMRouter.find_arb!"   the instances of test/cfmms.jl:64-107 (two-coin) and :117-199 (UniV3 fixture, 14 scenarios)
#   "arbitrage markets"                      test/arb.jl:41-89 with its feasibility predicates (:5-28), `all_flows .== netflows(r)` included
#   "swap markets"                           test/swap.jl:1-52
#   "README quick start"                     README.md:27-38
using CFMMRouter
using CFMMRouterAMD
using Test
using LinearAlgebra, Random, StatsBase

const CR = CFMMRouter
const FEAS_TOL = 1e-4                                   # test/arb.jl:3

# One pool, one price pair: the reference's per-pool method on the CPU (src/cfmms.jl:130-140, :185-196, :339-395).
function reference_trade(pool, v)
    Δ, Λ = zeros(2), zeros(2)
    CR.find_arb!(Δ, Λ, pool, v[pool.Ai])
    return Δ, Λ
end

# A vector of pools swept by the device at prices v (find_arb!(r::Router, v), src/router.jl:38-42), then compared row by
# row with the reference: `exact` families must agree in every bit, the others within `rtol` of the pool's reserve scale.
function device_matches_reference(pools, n, v; exact=true, rtol=1e-12)
    r = AMDRouter(LinearNonnegative(ones(n)), pools, n)
    find_arb!(r, v)
    for (i, pool) in enumerate(pools)
        Δ, Λ = reference_trade(pool, v)
        if exact
            @test r.Δs[i] == Δ
            @test r.Λs[i] == Λ
        else
            scale = max(1.0, maximum(pool.R))
            @test maximum(abs.(r.Δs[i] .- Δ)) <= rtol * scale
            @test maximum(abs.(r.Λs[i] .- Λ)) <= rtol * scale
        end
    end
    # Ψ: the device's reduction against the reference's serial loop over the reference's own rows
    ψ = zeros(n)
    for pool in pools
        Δ, Λ = reference_trade(pool, v)
        ψ[pool.Ai] .+= Λ .- Δ
    end
    @test maximum(abs.(netflows(r; exact=false) .- ψ)) <= 1e-12 * max(1.0, maximum(abs.(ψ)))
    exact && @test netflows(r) == ψ                       # exact = true (default): the reference's loop, bit for bit
    return r
end

# test/arb.jl:5-23 as predicates on an AMDRouter
function primal_feasible(r; arbitrage=true)
    flows = zero(r.v)
    for (Δ, Λ, pool) in zip(r.Δs, r.Λs, r.cfmms)
        @test all(Δ .>= -FEAS_TOL) && all(Λ .>= -FEAS_TOL)
        @test CR.ϕ(pool, R=pool.R + pool.γ * Δ - Λ) >= CR.ϕ(pool) - sqrt(eps())
        flows[pool.Ai] .+= Λ - Δ
    end
    @test all(flows .== netflows(r))                      # test/arb.jl:16, unedited semantics
    if arbitrage
        @test all(flows .>= -FEAS_TOL)
    else
        @test sum(flows .>= -FEAS_TOL) == 1
    end
end

# test/arb.jl:25-28
function dual_feasible(r)
    @test all(r.v .>= CR.lower_limit(r.objective) .- FEAS_TOL)
    @test all(r.v .<= CR.upper_limit(r.objective) .+ FEAS_TOL)
end

function random_product_market(npools, ncoins; seed=1234, fee=1.0)
    Random.seed!(seed)
    pools = Vector{CFMM{Float64}}(undef, npools)
    for i in 1:npools
        pools[i] = ProductTwoCoin(1000 * rand(2), fee, sample(1:ncoins, 2, replace=false))
    end
    return pools
end

@testset "CFMMRouterAMD" begin

@testset "device sweep vs CFMMRouter.find_arb!" begin
    Random.seed!(1234)
    fees = [rand() for _ in 1:3]
    reserves = [10 * rand(2) for _ in 1:3]
    prices = [rand(2) for _ in 1:3]

    @testset "ProductTwoCoin (bit for bit)" begin
        unit = ProductTwoCoin([1, 1], 1, [1, 2])
        for v in ([1.0, 1.0], [2.0, 2.0])                 # test/cfmms.jl:71-80: no arbitrage without a fee
            r = device_matches_reference(CFMM{Float64}[unit], 2, v)
            @test iszero(r.Δs[1]) && iszero(r.Λs[1])
        end
        r = device_matches_reference(CFMM{Float64}[unit], 2, [2.0, 1.0])          # test/cfmms.jl:82-86
        @test r.Δs[1][2] ≈ sqrt(2) - 1 && r.Λs[1][1] ≈ 1 - sqrt(1 / 2)
        pools = CFMM{Float64}[ProductTwoCoin(R, γ, [1, 2]) for R in reserves for γ in fees]
        for v in prices
            device_matches_reference(pools, 2, v)
        end
        @test_throws ArgumentError AMDRouter(LinearNonnegative(ones(2)), CFMM{Float64}[ProductTwoCoin([1, 1], 1, [1, 3])], 2)
    end

    @testset "GeometricMeanTwoCoin (log-space forms: 1e-12 of the reserve scale)" begin
        weights = [(w = rand(); [w, 1 - w]) for _ in 1:3]
        pools = CFMM{Float64}[GeometricMeanTwoCoin(R, w, γ, [1, 2]) for R in reserves for γ in fees for w in weights]
        for v in prices
            device_matches_reference(pools, 2, v; exact=false)
        end
        # option geomean_exact = 1: pow in the reference's operation order (device libm's pow: within 1e-12 as well)
        r = AMDRouter(LinearNonnegative(ones(2)), pools, 2)
        CFMMRouterAMD.set_option!(r, "geomean_exact", 1)
        find_arb!(r, prices[1])
        for (i, pool) in enumerate(pools)
            Δ, Λ = reference_trade(pool, prices[1])
            @test maximum(abs.(r.Δs[i] .- Δ)) <= 1e-12 * max(1.0, maximum(pool.R))
        end
    end

    @testset "UniV3 fixture (bit for bit)" begin
        # the reference's hand fixture (test/cfmms.jl:117-120) and its fourteen price scenarios (:127-199)
        for γ in (1.0, 0.997)
            pool = UniV3(15.0, [30.0, 20, 10, 5], [1.0, 2.0, 1.5, 0.0], γ, [1, 2])
            inside = γ == 1.0 ? 15.0 : 15.0 * (1 + γ) / 2
            for p in (inside, 16.0, 14.0, 25.0, 7.5, 4.0, 35.0)
                device_matches_reference(CFMM{Float64}[pool], 2, [p, 1.0])
            end
        end
    end

    @testset "mixed families in one router, shuffled" begin
        Random.seed!(7)
        n = 6
        pools = CFMM{Float64}[]
        for _ in 1:40
            Ai = sample(1:n, 2, replace=false)
            push!(pools, ProductTwoCoin(1000 * rand(2), rand((0.997, 1.0)), Ai))
            w = rand()
            push!(pools, GeometricMeanTwoCoin(1000 * rand(2), [w, 1 - w], 0.997, Ai))
            push!(pools, UniV3(15.0, [30.0, 20, 10, 5], [1.0, 2.0, 1.5, 0.0], 0.997, Ai))
        end
        shuffle!(pools)
        v = exp.(0.3 .* (2 .* rand(n) .- 1))
        r = AMDRouter(LinearNonnegative(ones(n)), pools, n)
        find_arb!(r, v)
        for (i, pool) in enumerate(pools)                   # router order is the caller's order, whatever the packing
            Δ, Λ = reference_trade(pool, v)
            if pool isa GeometricMeanTwoCoin
                @test maximum(abs.(r.Δs[i] .- Δ)) <= 1e-9
            else
                @test r.Δs[i] == Δ && r.Λs[i] == Λ
            end
        end
    end
end

@testset "arbitrage markets" begin
    @testset "two pools" begin
        r = AMDRouter(LinearNonnegative(ones(2)), CFMM{Float64}[ProductTwoCoin([100, 100], 1, [1, 2]), ProductTwoCoin([1, 2], 1, [1, 2])], 2)
        route!(r)
        primal_feasible(r)
        dual_feasible(r)
    end
    @testset "100 random pools, 10 coins, no fee" begin
        pools = random_product_market(100, 10)
        c = rand(10)
        r = AMDRouter(LinearNonnegative(c), pools, 10)
        route!(r)
        primal_feasible(r)
        dual_feasible(r)
        # the same market through the reference's Router: same solver (LBFGSB.jl), same callbacks up to summation order
        ref = Router(LinearNonnegative(c), pools, 10)
        route!(ref)
        @test maximum(abs.(netflows(r) .- netflows(ref))) <= 1e-6 * maximum(abs.(netflows(ref)))     # north_star's tolerance
        # ... and through the library's own L-BFGS-B (one ccall for the whole route!)
        rn = AMDRouter(LinearNonnegative(c), pools, 10)
        info = route_native!(rn)
        @test info.evaluations >= 2
        @test maximum(abs.(netflows(rn) .- netflows(ref))) <= 1e-6 * maximum(abs.(netflows(ref)))
        primal_feasible(rn)
        dual_feasible(rn)
    end
end

@testset "swap markets" begin
    @testset "two pools" begin
        r = AMDRouter(BasketLiquidation(1, [5.0, 0.0]), CFMM{Float64}[ProductTwoCoin([100, 100], 1, [1, 2]), ProductTwoCoin([1, 2], 1, [1, 2])], 2)
        route!(r)
        primal_feasible(r)
        dual_feasible(r)
    end
    @testset "100 random pools, 10 coins, no fee" begin
        pools = random_product_market(100, 10)
        Δin = vcat([0.0], 100 * rand(9))
        r = AMDRouter(BasketLiquidation(1, Δin), pools, 10)
        route!(r)
        primal_feasible(r; arbitrage=false)
        dual_feasible(r)
        ref = Router(BasketLiquidation(1, Δin), pools, 10)
        route!(ref)
        @test maximum(abs.(netflows(r) .- netflows(ref))) <= 1e-6 * maximum(abs.(netflows(ref)))
    end
end

@testset "README quick start" begin
    pools = CFMM{Float64}[ProductTwoCoin([1e6, 1e6], 1, [1, 2]), ProductTwoCoin([1e3, 2e3], 1, [1, 2])]
    r = AMDRouter(LinearNonnegative(ones(2)), pools, 2)
    route!(r)
    Ψ = netflows(r)
    @test abs(Ψ[1]) <= 1e-3 && isapprox(Ψ[2], 171.4; atol=0.1)
    rn = AMDRouter(LinearNonnegative(ones(2)), pools, 2)
    route_native!(rn)
    @test isapprox(netflows(rn)[2], Ψ[2]; rtol=1e-6)
end

@testset "update_reserves!: no arbitrage left at the same prices" begin
    pools = random_product_market(200, 8; seed=99, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    route!(r)
    v = copy(r.v)
    before = [copy(p.R) for p in r.cfmms]
    traded = [copy(Δ) for Δ in r.Δs], [copy(Λ) for Λ in r.Λs]
    update_reserves!(r)
    for (i, p) in enumerate(r.cfmms)                       # R <- R + γΔ − Λ (src/cfmms.jl:26-31)
        @test p.R ≈ before[i] .+ p.γ .* traded[1][i] .- traded[2][i]
    end
    find_arb!(r, v)
    @test all(maximum(abs.(Δ)) <= 1e-9 for Δ in r.Δs)
end

@testset "select_trades: the pools that trade, selected on the device" begin
    pools = random_product_market(300, 8; seed=7, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    v = rand(8) .+ 0.5
    find_arb!(r, v)
    value(i) = foldl((acc, k) -> acc + (r.Λs[i][k] - r.Δs[i][k]) * v[pools[i].Ai[k]], 1:2; init=0.0)
    for τ in (-Inf, 0.0, 1.0)
        want = [i for i in 1:300 if (any(r.Δs[i] .!= 0) || any(r.Λs[i] .!= 0)) && !(value(i) < τ)]
        idx, Δ, Λ, val = select_trades(r, 0; min_value=τ)        # one ProductTwoCoin segment: its rows are r.order
        @test r.order[idx] == want
        @test all(Δ[:, j] == r.Δs[want[j]] && Λ[:, j] == r.Λs[want[j]] && val[j] == value(want[j]) for j in eachindex(want))
        @test length(select_trades(r, 0; min_value=τ, capacity=0)[1]) == 0
    end
end

@testset "quote_swaps_out: the input for a wanted output, the inverse of quote_swaps" begin
    pools = random_product_market(50, 8; seed=9, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    which = collect(1:50)
    cin = [1 + i % 2 for i in which]
    want = [0.1 * pools[i].R[3 - cin[i]] for i in which]                 # a tenth of the other reserve
    a = quote_swaps_out(r, which, cin, want)
    @test all(a[i] ≈ pools[i].R[cin[i]] * want[i] / ((pools[i].R[3 - cin[i]] - want[i]) * 0.997) for i in which)
    @test all(isapprox.(quote_swaps(r, which, cin, a), want; rtol=1e-12))
    @test quote_swaps_out(r, [1], [1], [2 * pools[1].R[2]])[1] == Inf       # more than the pool holds: not an error
    @test backward_trade([0.0, want[1]], pools[1]) ≈ a[1] || cin[1] != 1
    @test backward_trade([0.0, 0.0], pools[1]) == 0.0
end


@testset "quote_paths / quote_paths_out: an amount through a path of pools, hop by hop on the pools as they stand" begin
    pools = random_product_market(50, 8; seed=10, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    # two-hop paths through pools that share a token
    pairs = [(i, j) for i in 1:50 for j in 1:50 if i != j && pools[i].Ai[2] == pools[j].Ai[1]][1:min(end, 20)]
    paths = [[i, j] for (i, j) in pairs]
    toks = [[pools[i].Ai[1], pools[i].Ai[2], pools[j].Ai[2]] for (i, j) in pairs]
    a = [0.05 * pools[i].R[1] for (i, _) in pairs]
    out, hv = quote_paths(r, paths, toks, a; hops=true)
    mid = quote_swaps(r, [i for (i, _) in pairs], fill(1, length(pairs)), a)
    @test hv[:, 1] == mid                                                     # the bits of chaining the single-pool quote
    @test out == quote_swaps(r, [j for (_, j) in pairs], fill(1, length(pairs)), mid) && hv[:, 2] == out
    back = quote_paths_out(r, paths, toks, 0.5 .* out)
    @test all(back .< a)
    @test_throws ArgumentError quote_paths(r, [[1, 1]], [[pools[1].Ai[1], pools[1].Ai[2], pools[1].Ai[1]]], [1.0])
end

@testset "find_paths: the best path between two tokens, found on the device, then quoted and executed" begin
    pools = random_product_market(50, 8; seed=11, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    tin = [1 + q % 8 for q in 0:15]; tout = [1 + (q + 3) % 8 for q in 0:15]
    a = fill(0.01 * pools[1].R[1], 16)
    out, paths, toks, status = find_paths(r, tin, tout, a; max_hops=3)
    found = findall(==(0), status)
    @test !isempty(found)
    @test all(toks[q][1] == tin[q] && toks[q][end] == tout[q] && length(toks[q]) == length(paths[q]) + 1 for q in found)
    @test quote_paths(r, paths[found], toks[found], a[found]) == out[found]      # the bits of quoting the found path
    q = found[1]
    got, st = swap_paths!(r, [paths[q]], [toks[q]], [a[q]]; min_out=[out[q]])
    @test st == [0] && got[1] == out[q]
    @test find_paths(r, [tin[q]], [tout[q]], [a[q]]; max_hops=3)[1][1] < out[q]   # the same query afterwards: a worse price
    @test find_paths(r, [1], [2], [0.0])[4] == [1]                                # nothing to carry: not found
    @test_throws ArgumentError find_paths(r, [9], [1], [1.0])
end

@testset "find_paths_out: the cheapest path that buys an exact amount, found on the device, then quoted and executed" begin
    pools = random_product_market(50, 8; seed=12, fee=0.997)
    r = AMDRouter(LinearNonnegative(rand(8)), pools, 8)
    tin = [1 + q % 8 for q in 0:15]; tout = [1 + (q + 3) % 8 for q in 0:15]
    want = fill(1e-3 * minimum(minimum(p.R) for p in pools), 16)
    cost, paths, toks, status = find_paths_out(r, tin, tout, want; max_hops=3)
    found = findall(==(0), status)
    @test !isempty(found)
    @test all(toks[q][1] == tin[q] && toks[q][end] == tout[q] && length(toks[q]) == length(paths[q]) + 1 for q in found)
    @test quote_paths_out(r, paths[found], toks[found], want[found]) == cost[found]   # the bits of quoting the found path
    q = found[1]
    paid, st = swap_paths_out!(r, [paths[q]], [toks[q]], [want[q]]; max_in=[cost[q]])
    @test st == [0] && paid[1] == cost[q]
    @test find_paths_out(r, [tin[q]], [tout[q]], [want[q]]; max_hops=3)[1][1] > cost[q]   # the same order afterwards: dearer
    none = find_paths_out(r, [1, 1], [2, 2], [0.0, 1e300])
    @test none[4] == [1, 1] && none[1] == [0.0, Inf]                           # nothing to buy; more than any pool holds
    @test_throws ArgumentError find_paths_out(r, [9], [1], [1.0])
end

@testset "size_paths: the input of a cycle that maximises its gain, then executed" begin
    pools = [ProductTwoCoin([1.00e5, 2.00e5], 0.997, [1, 2]), ProductTwoCoin([2.00e5, 1.04e5], 0.997, [2, 3]),
             ProductTwoCoin([1.0e5, 1.0e5], 0.9995, [3, 1])]
    r = AMDRouter(LinearNonnegative(ones(3)), pools, 3)
    cycle, toks = [1, 2, 3], [1, 2, 3, 1]
    x, y, g, st = size_paths(r, [cycle, cycle], [toks, toks], [5000.0, 10.0])
    @test st == [0, 2] && x[2] == 10.0 && 0 < x[1] < 5000.0                  # sized inside the limit; the small limit binds
    @test quote_paths(r, [cycle, cycle], [toks, toks], x) == y               # the bits of quoting the answer
    @test g == y .- x && all(g .> 0)
    sizes = 50.0 .* 1.25 .^ (0:19)
    ladder = quote_paths(r, fill(cycle, 20), fill(toks, 20), sizes) .- sizes
    @test g[1] >= maximum(ladder)                                            # at least the best of a hand-made ladder
    got, applied = swap_paths!(r, [cycle], [toks], [x[1]]; min_out=[x[1]])
    @test applied == [0] && got[1] == y[1]
    again = size_paths(r, [cycle], [toks], [5000.0])
    @test again[4][1] == 1 || again[3][1] < 1e-3 * g[1]                      # the market it left: nothing, or next to nothing
    @test size_paths(r, [cycle], [toks], [100.0]; value_in=[2.0])[4] == [1]  # the input valued at twice the output: no size gains
    @test_throws ArgumentError size_paths(r, [cycle], [toks], [100.0]; rounds=17)
    @test_throws ArgumentError size_paths(r, [[1, 1]], [[1, 2, 1]], [100.0])
end
end
