// ladder_store_host.cpp -- csrc/ladder_store.h (the host's tick ladders of a UniV3 segment) driven on the CPU against a plain
// list-of-vectors model: thousands of random replace / shrink / grow / re-tighten steps, the store compared with the model
// after each.  A stand-alone program: tests/test_pool_ticks_cpu.py builds it with -fsanitize=address,undefined and runs it.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cfmmrouter.jl_amd/csrc ladder_store_host.cpp
#include "ladder_store.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using cfmm::LadderStore;

namespace {

struct Model {
    std::vector<std::vector<double>> lt, lq;
};

int fail(const char* what, long step)
{
    std::fprintf(stderr, "ladder store: %s at step %ld\n", what, step);
    return 1;
}

bool same(const LadderStore& s, const Model& m, int64_t i)
{
    if (s.count(i) != (int64_t)m.lt[(size_t)i].size()) return false;
    for (int64_t j = 0; j < s.count(i); ++j)
        if (s.lower_ticks(i)[j] != m.lt[(size_t)i][(size_t)j] || s.liquidity(i)[j] != m.lq[(size_t)i][(size_t)j]) return false;
    return true;
}

bool same_all(LadderStore& s, const Model& m, bool through_csr)
{
    int64_t total = 0;
    for (const auto& v : m.lt) total += (int64_t)v.size();
    if (s.ticks_total() != total || s.pools() != (int64_t)m.lt.size()) return false;
    if (s.ticks_held() < total || s.ticks_held() - total > total / 2 + 4096 + 130) return false;   // the garbage bound (+ one ladder)
    if (!through_csr) {
        for (int64_t i = 0; i < s.pools(); ++i)
            if (!same(s, m, i)) return false;
        return true;
    }
    const LadderStore::Csr c = s.csr();
    if (s.ticks_held() != total || c.tick_off[0] != 0 || c.tick_off[s.pools()] != total) return false;
    for (int64_t i = 0; i < s.pools(); ++i) {
        const int64_t o = c.tick_off[i], n = c.tick_off[i + 1] - o;
        if (n != (int64_t)m.lt[(size_t)i].size()) return false;
        for (int64_t j = 0; j < n; ++j)
            if (c.lower_ticks[o + j] != m.lt[(size_t)i][(size_t)j] || c.liquidity[o + j] != m.lq[(size_t)i][(size_t)j]) return false;
        if (!same(s, m, i)) return false;
    }
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    const long steps = argc > 1 ? std::atol(argv[1]) : 20000;
    std::mt19937_64 rng(20240607);
    auto uni = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    auto ladder = [&](int64_t n, std::vector<double>& lt, std::vector<double>& lq) {
        lt.resize((size_t)n);
        lq.resize((size_t)n);
        for (int64_t j = 0; j < n; ++j) {
            lt[(size_t)j] = (double)(rng() >> 11);
            lq[(size_t)j] = (double)(rng() >> 11);
        }
    };
    for (int round = 0; round < 3; ++round) {
        const int64_t m = round == 0 ? 1 : round == 1 ? 37 : 600;
        Model model;
        model.lt.resize((size_t)m);
        model.lq.resize((size_t)m);
        std::vector<int64_t> off(1, 0);
        std::vector<double> lt, lq;
        for (int64_t i = 0; i < m; ++i) {
            ladder(uni(1, 64), model.lt[(size_t)i], model.lq[(size_t)i]);
            lt.insert(lt.end(), model.lt[(size_t)i].begin(), model.lt[(size_t)i].end());
            lq.insert(lq.end(), model.lq[(size_t)i].begin(), model.lq[(size_t)i].end());
            off.push_back((int64_t)lt.size());
        }
        LadderStore s;
        s.assign(m, off.data(), lt.data(), lq.data());
        std::vector<double>().swap(lt);   // (the store keeps its own copy)
        std::vector<double>().swap(lq);
        if (!same_all(s, model, true)) return fail("assign", -1);
        for (long step = 0; step < steps; ++step) {
            const int64_t i = uni(0, m - 1), old = s.count(i);
            const int kind = (int)uni(0, 5);
            // same length, shrink (down to one tick), grow (up to 128), anything, one tick, a burst on one pool
            const int64_t n = kind == 0 ? old : kind == 1 ? uni(1, old) : kind == 2 ? uni(old, 128) : kind == 3 ? uni(1, 128) : kind == 4 ? 1 : uni(100, 128);
            std::vector<double> a, b;
            ladder(n, a, b);
            s.replace(i, n, a.data(), b.data());
            model.lt[(size_t)i] = a;
            model.lq[(size_t)i] = b;
            if (!same(s, model, i)) return fail("the replaced ladder differs", step);
            if (step % 97 == 0 && !same_all(s, model, false)) return fail("a ladder differs", step);
            if (step % 1013 == 0 && !same_all(s, model, true)) return fail("the CSR form differs", step);
        }
        if (!same_all(s, model, true)) return fail("the final CSR form differs", steps);
    }
    std::printf("LADDER_STORE_OK %ld steps x 3 markets\n", steps);
    return 0;
}
