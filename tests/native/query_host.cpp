// Host build of what the query entries share (csrc/stage_layout.h, shard_split.h, seg_view.h, hostres.h EventPairs) for
// tests/test_query_host_cpu.py: a stand-alone program, built with the address and undefined-behaviour sanitizers.  Not linked
// against the HIP runtime: the raw create / destroy calls of the owners are defined HERE over malloc / free (a freed "device
// array" is never handed out again, so a regrown DevBuf always shows a new address).  Nothing touches a GPU.
#include "kind_switch.h"
#include "seg_view.h"
#include "shard_split.h"
#include "stage_layout.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cfmm;

static std::vector<void*> g_freed;

namespace cfmm {
hipError_t dev_alloc(void** p, size_t bytes) { return (*p = std::malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory; }
hipError_t dev_alloc_fine(void** p, size_t bytes) { return dev_alloc(p, bytes); }
void dev_free(void* p) { g_freed.push_back(p); }
hipError_t pinned_alloc(void** h, void** d, size_t bytes, bool) { *d = nullptr; return dev_alloc(h, bytes); }
void pinned_free(void* h) { std::free(h); }
hipError_t event_create(hipEvent_t* e, unsigned) { *e = static_cast<hipEvent_t>(std::malloc(1)); return hipSuccess; }
void event_destroy(hipEvent_t e) { std::free(e); }
hipError_t stream_create(hipStream_t* s) { *s = nullptr; return hipErrorNotSupported; }
void stream_destroy(hipStream_t) {}
int fail(const cfmm_ctx*, int code, const char*, ...) { return code; }
} // namespace cfmm
extern "C" const char* hipGetErrorString(hipError_t) { return "injected failure"; }
extern "C" hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.5f; return hipSuccess; }

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
            return 1;                                                    \
        }                                                                \
    } while (0)

// ---- StageLayout ----------------------------------------------------------------------------------------------------------

struct Span { size_t off, words; };

// writes column `c` to its end inside `st` (ASan judges the heap buffer) and notes the words it takes
template <class T>
void touch(const StageCol<T>& c, unsigned long long* st, std::vector<Span>& spans)
{
    if (c.n) std::memset(c.in(st), 0x5a, c.n * sizeof(T));
    spans.push_back({c.off, words_of(c.n * sizeof(T))});
}

// every column of one layout: inside a heap buffer of exactly words() words, on word boundaries by construction of `in`,
// no two overlapping, the last one ending at words()
template <class Touch>
int check_layout(size_t words, Touch touch_all)
{
    std::vector<unsigned long long> heap(words);   // (exactly `words`: one word more written and ASan reports it)
    unsigned long long* st = heap.data();
    std::vector<Span> spans;
    touch_all(st, spans);
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.off != b.off ? a.off < b.off : a.words < b.words; });
    size_t end = 0;
    for (const Span& s : spans) {
        CHECK(s.off >= end);           // starts behind everything before it (an empty column may share its start)
        end = s.off + s.words;
    }
    CHECK(end == words);
    return 0;
}

int test_layouts()
{
    const size_t counts[] = {0, 1, 2, 3, 65}, hops[] = {1, 3, 8}, recs[] = {1, 3};
    CHECK(words_of(0) == 0 && words_of(1) == 1 && words_of(8) == 1 && words_of(9) == 2 && words_of(4 * 65) == 33);
    for (size_t n : counts) {
        for (int opt = 0; opt < 16; ++opt) {
            const bool o0 = opt & 1, o1 = opt & 2, o2 = opt & 4, o3 = opt & 8;
            const QuoteStage q(n, o0);
            CHECK(q.idx.n == (o0 ? n : 0) && q.coins.n == 2 * n);
            CHECK(!check_layout(q.l.words(), [&](unsigned long long* st, std::vector<Span>& sp) {
                touch(q.amt, st, sp); touch(q.coins, st, sp); touch(q.out, st, sp); touch(q.idx, st, sp);
            }));
            const SwapStage s(n, o0, o1, o2, o3);
            CHECK(s.price.n == (o1 ? n : 0) && s.limit.n == (o2 ? n : 0) && s.status.n == (o3 ? n : 0) && s.left.n == 1);
            CHECK(!check_layout(s.l.words(), [&](unsigned long long* st, std::vector<Span>& sp) {
                touch(s.amt, st, sp); touch(s.coins, st, sp); touch(s.out, st, sp); touch(s.price, st, sp); touch(s.idx, st, sp);
                touch(s.limit, st, sp); touch(s.status, st, sp); touch(s.left, st, sp);
            }));
        }
        for (size_t H : hops)
            for (size_t nrec : recs) {
                const size_t nh = n * H;
                for (int want = 0; want < 2; ++want) {
                    const PathStage p(nrec * sizeof(PathSeg), n, nh, want != 0);
                    CHECK(p.table.off == 0 && p.i32.n == n + 3 * nh && p.hops.n == (want ? nh : 0));
                    CHECK(!check_layout(p.l.words(), [&](unsigned long long* st, std::vector<Span>& sp) {
                        touch(p.table, st, sp); touch(p.i32, st, sp); touch(p.row, st, sp); touch(p.given, st, sp); touch(p.answer, st, sp);
                        touch(p.hops, st, sp);
                    }));
                }
                const SwapPathStage w(nrec * sizeof(SwapPathSeg), nrec, n, nh);
                CHECK(w.table.off == 0 && w.amt.n == 2 * n && w.left.n == nrec);
                CHECK(!check_layout(w.l.words(), [&](unsigned long long* st, std::vector<Span>& sp) {
                    touch(w.table, st, sp); touch(w.i32, st, sp); touch(w.row, st, sp); touch(w.amt, st, sp); touch(w.out, st, sp);
                    touch(w.hops, st, sp); touch(w.price, st, sp); touch(w.status, st, sp); touch(w.left, st, sp);
                }));
                const FindStage f(nrec * sizeof(FindSeg), n, nh);
                CHECK(f.table.off == 0 && f.tok.n == 2 * n && f.ns.n == 2 * n && f.hop32.n == 3 * nh);
                CHECK(!check_layout(f.l.words(), [&](unsigned long long* st, std::vector<Span>& sp) {
                    touch(f.table, st, sp); touch(f.tok, st, sp); touch(f.amt, st, sp); touch(f.out, st, sp); touch(f.ns, st, sp);
                    touch(f.hop32, st, sp); touch(f.row, st, sp);
                }));
            }
    }
    // the rounding, spelled out once: 65 paths of 3 hops -> 65 + 585 int32 = 325 words, behind a one-record table of 16 words
    const PathStage p(sizeof(PathSeg), 65, 195, true);
    CHECK(p.i32.off == 16 && p.row.off == 16 + 325 && p.given.off == p.row.off + 195 && p.l.words() == p.given.off + 65 + 65 + 195);
    return 0;
}

// ---- the shard split ------------------------------------------------------------------------------------------------------

int test_split()
{
    const int64_t ms[] = {0, 1, 5, 64, 1000};
    const int nds[] = {1, 2, 3, 8};
    for (int64_t m : ms)
        for (int nd : nds) {
            // the ranges tile [0, m) in device order
            int64_t next = 0;
            for (int d = 0; d < nd; ++d) {
                int64_t lo, hi;
                shard_range(m, d, nd, lo, hi);
                CHECK(lo == next && hi >= lo && hi - lo <= m / nd + 1);
                next = hi;
            }
            CHECK(next == m);
            for (int with_idx = 0; with_idx < 2; ++with_idx) {
                std::vector<int64_t> idx;   // unordered, with repeats
                for (int64_t q = 0; with_idx && m > 0 && q < 2 * m + 3; ++q) idx.push_back((q * 7919 + (q % 3) * 31) % m);
                const int64_t count = with_idx ? (int64_t)idx.size() : m;
                const std::vector<ShardBucket> b = split_by_shard(m, nd, count, with_idx ? idx.data() : nullptr);
                CHECK((int)b.size() == nd);
                std::vector<double> col((size_t)count), back((size_t)count, -1.0);
                std::vector<int32_t> coin((size_t)count), coin_back((size_t)count, -1);
                for (int64_t q = 0; q < count; ++q) { col[(size_t)q] = 0.25 * (double)q; coin[(size_t)q] = (int32_t)(q % 5); }
                int64_t seen = 0;
                for (int d = 0; d < nd; ++d) {
                    int64_t lo, hi;
                    shard_range(m, d, nd, lo, hi);
                    // brute force: the queries whose row lies in this shard's range, in the caller's order
                    std::vector<int64_t> where, rows;
                    for (int64_t q = 0; q < count; ++q) {
                        const int64_t row = with_idx ? idx[(size_t)q] : q;
                        if (row >= lo && row < hi) { where.push_back(q); rows.push_back(row - lo); }
                    }
                    CHECK(b[(size_t)d].where == where && b[(size_t)d].rows == rows);
                    CHECK(std::is_sorted(where.begin(), where.end()));
                    seen += (int64_t)where.size();
                    const std::vector<double> g = gather(where, col.data());
                    const std::vector<int32_t> gc = gather(where, coin.data());
                    CHECK(g.size() == where.size() && gather(where, (const double*)nullptr).empty());
                    for (size_t j = 0; j < where.size(); ++j) CHECK(g[j] == col[(size_t)where[j]] && gc[j] == coin[(size_t)where[j]]);
                    scatter(where, g.data(), back.data());
                    scatter(where, gc.data(), coin_back.data());
                }
                CHECK(seen == count && back == col && coin_back == coin);
            }
        }
    return 0;
}

// ---- the segment views ----------------------------------------------------------------------------------------------------

// a segment of `kind` with EVERY device array of every kind allocated: a view that took a member of another kind would show
void fill(Segment& s, int kind, int64_t m, int n_coins)
{
    s.kind = kind;
    s.m = m;
    s.n_coins = n_coins;
    const size_t k = 4;
    s.R.alloc(nullptr, k); s.w.alloc(nullptr, k); s.gamma.alloc(nullptr, k); s.eta.alloc(nullptr, k); s.lR.alloc(nullptr, k);
    s.Ai.alloc(nullptr, k); s.pk.alloc(nullptr, k);
    s.u.pg.alloc(nullptr, k); s.u.cp.alloc(nullptr, k); s.u.cur_a.alloc(nullptr, k); s.u.cur_b.alloc(nullptr, k); s.u.cur_c.alloc(nullptr, k);
    s.u.curR.alloc(nullptr, k); s.u.walk.alloc(nullptr, k); s.u.ticks.alloc(nullptr, k); s.u.thr.alloc(nullptr, k); s.u.head.alloc(nullptr, k);
    s.nc.R.alloc(nullptr, k); s.nc.q.alloc(nullptr, k); s.nc.tok.alloc(nullptr, k); s.nc.glg.alloc(nullptr, k); s.nc.par.alloc(nullptr, k);
    s.nc.D.alloc(nullptr, k); s.nc.L.alloc(nullptr, k);
}

int check_views(const Segment& s, int* left)
{
    const bool ragged = ragged_kind(s.kind), univ3 = s.kind == CFMM_KIND_UNIV3, two = !ragged && !univ3;
    const PathSeg p = path_seg(s);
    CHECK(p.kind == (s.m > 0 ? s.kind : -1) && p.m == s.m && p.n_coins == (ragged ? s.n_coins : 2));
    CHECK(p.R == (two ? s.R.get() : nullptr) && p.w == (two ? s.w.get() : nullptr) && p.gamma == (two ? s.gamma.get() : nullptr));
    CHECK(p.pg == (univ3 ? s.u.pg.get() : nullptr) && p.cur_a == (univ3 ? s.u.cur_a.get() : nullptr) && p.cur_b == (univ3 ? s.u.cur_b.get() : nullptr));
    CHECK(p.cur_c == (univ3 ? s.u.cur_c.get() : nullptr) && p.curR == (univ3 ? s.u.curR.get() : nullptr));
    CHECK(p.walk == (univ3 ? s.u.walk.get() : nullptr) && p.ticks == (univ3 ? s.u.ticks.get() : nullptr));
    CHECK(p.nR == (ragged ? s.nc.R.get() : nullptr) && p.nq == (ragged ? s.nc.q.get() : nullptr));
    CHECK(p.nglg == (ragged ? s.nc.glg.get() : nullptr) && p.npar == (ragged ? s.nc.par.get() : nullptr));
    // the single-segment views, pointer for pointer
    QuoteArgs a{};
    quote_view(p, a);
    CHECK(a.m == p.m && a.n_coins == p.n_coins && a.R == p.R && a.w == p.w && a.gamma == p.gamma);
    const UniV3Pools u = univ3_view(p);
    CHECK(u.pg == p.pg && u.cur_a == p.cur_a && u.cur_b == p.cur_b && u.cur_c == p.cur_c && u.curR == p.curR && u.walk == p.walk && u.ticks == p.ticks);
    CHECK(!u.Ai && !u.thr && !u.head && !u.has_walk && !u.cp && !u.pk && !u.gbase);
    const NCoinPools n = ncoin_view(p);
    CHECK(n.R == p.nR && n.q == p.nq && n.glg == p.nglg && n.par == p.npar && n.n_coins == (ragged ? s.n_coins : 0));
    CHECK(!n.tok && !n.Delta && !n.Lambda);
    // the swaps' and the search's records carry the same view
    const SwapPathSeg w = swap_path_seg(s, left);
    CHECK(std::memcmp(&w.s, &p, sizeof p) == 0);
    CHECK(w.R == (two ? s.R.get() : nullptr) && w.Q == (two ? s.lR.get() : nullptr) && w.eta == (two ? s.eta.get() : nullptr));
    CHECK(w.nR == (ragged ? s.nc.R.get() : nullptr) && w.nq == (ragged ? s.nc.q.get() : nullptr));
    CHECK(w.left_window == (two && kind_info(s.kind).has_fast ? left : nullptr) && w.pad[0] == 0 && w.pad[1] == 0);
    SwapArgs sa{};
    swap_view(w, sa);
    CHECK(sa.q.R == p.R && sa.q.m == p.m && sa.R == w.R && sa.Q == w.Q && sa.eta == w.eta && sa.ncR == w.nR && sa.ncq == w.nq && sa.left_window == w.left_window);
    const FindSeg f = find_seg(s, 7, 11);
    CHECK(std::memcmp(&f.s, &p, sizeof p) == 0 && f.first_tile == 7 && f.first_pool == 11);
    CHECK(f.tok == (ragged ? s.nc.tok.get() : nullptr) && f.pk == (ragged ? nullptr : s.pk.get()) && f.Ai == (ragged ? nullptr : s.Ai.get()));
    return 0;
}

int test_views()
{
    int left[8] = {};
    cfmm_ctx c, parent;
    const int kinds[] = {CFMM_KIND_PRODUCT, CFMM_KIND_GEOMEAN, CFMM_KIND_UNIV3, CFMM_KIND_WEIGHTED, CFMM_KIND_CURVE, CFMM_KIND_SOLIDLY, CFMM_KIND_GEOMEAN};
    for (size_t i = 0; i < 7; ++i) {
        c.segs.emplace_back();
        fill(c.segs.back(), kinds[i], i == 6 ? 0 : 10 + (int64_t)i, ragged_kind(kinds[i]) ? 3 : 2);   // the last one: no pools
        CHECK(!check_views(c.segs.back(), left + i));
        parent.psegs.push_back({kinds[i], 20 + (int64_t)i, 0, ragged_kind(kinds[i]) ? 4 : 7, 0});   // (n_coins of a two-coin kind: ignored)
    }
    CHECK(path_seg(c.segs[6]).kind == -1);
    // a regrown array shows in the next view (and only there)
    const PathSeg before = path_seg(c.segs[2]);
    c.segs[2].u.ticks.alloc(nullptr, 64);
    c.segs[3].nc.R.alloc(nullptr, 64);
    CHECK(path_seg(c.segs[2]).ticks == c.segs[2].u.ticks.get() && path_seg(c.segs[2]).ticks != before.ticks && path_seg(c.segs[2]).pg == before.pg);
    CHECK(!check_views(c.segs[2], left) && !check_views(c.segs[3], left));
    // the segment as the checks see it: a single context reads its segments, a parent its own list
    parent.shards.push_back(nullptr);
    CHECK(seg_count(&c) == 7 && seg_count(&parent) == 7);
    const std::vector<PathSegInfo> si = seg_infos(&c), pi = seg_infos(&parent);
    for (size_t i = 0; i < 7; ++i) {
        const bool ragged = ragged_kind(kinds[i]);
        CHECK(si[i].kind == kinds[i] && si[i].m == c.segs[i].m && si[i].n_coins == (ragged ? 3 : 2));
        CHECK(pi[i].kind == kinds[i] && pi[i].m == 20 + (int64_t)i && pi[i].n_coins == (ragged ? 4 : 2));
        CHECK(seg_info(&parent, (int32_t)i).m == pi[i].m && seg_info(&c, (int32_t)i).n_coins == si[i].n_coins);
    }
    // the tables: one record per segment; a context without pools: one record of kind -1 with two coins
    std::vector<SwapPathSeg> t(table_records(&c));
    CHECK(t.size() == 7);
    build_table(&c, t.data(), [&](const Segment& s, size_t i) { return swap_path_seg(s, left + i); });
    for (size_t i = 0; i < 7; ++i) {
        const SwapPathSeg w = swap_path_seg(c.segs[i], left + i);
        CHECK(std::memcmp(&t[i], &w, sizeof w) == 0);
    }
    cfmm_ctx empty;
    PathSeg one;
    std::memset(&one, 0xff, sizeof one);
    CHECK(table_records(&empty) == 1);
    build_table(&empty, &one, [](const Segment& s, size_t) { return path_seg(s); });
    CHECK(one.kind == -1 && one.n_coins == 2 && one.m == 0 && !one.R && !one.pg && !one.nR && !one.npar);
    return 0;
}

// ---- the event pairs ------------------------------------------------------------------------------------------------------

int test_event_pairs()
{
    EventPairs ev;
    CHECK(ev.start(3, false) == nullptr && ev.stop(3, false) == nullptr);   // timing off: nulls, whatever exists
    CHECK(ev.ensure(nullptr, 2) == CFMM_OK && ev.ev.size() == 4);
    const hipEvent_t a = ev.start(0), b = ev.stop(1);
    CHECK(a && b && a != ev.stop(0));
    CHECK(ev.ensure(nullptr, 3, 2) == CFMM_OK && ev.ev.size() == 6 && ev.start(0) == a && ev.stop(1) == b && ev.start(2));   // kept
    CHECK(ev.ensure(nullptr, 1) == CFMM_OK && ev.ev.size() == 6);
    int64_t ns = -1;
    CHECK(ev.elapsed_ns(nullptr, 1, 1, ns) == CFMM_OK && ns == 500000);
    CHECK(ev.elapsed_ns(nullptr, 0, 3, ns) == CFMM_OK && ns == 1500000);
    return 0;
}

// ---- the kind dispatch ----------------------------------------------------------------------------------------------------

// every kind reaches f exactly once, with its own constant; a number that names no kind reaches `none`
int test_with_kind()
{
    const int kinds[] = {CFMM_KIND_PRODUCT, CFMM_KIND_GEOMEAN, CFMM_KIND_UNIV3, CFMM_KIND_WEIGHTED, CFMM_KIND_CURVE, CFMM_KIND_SOLIDLY};
    for (int kind : kinds) {
        int calls = 0, seen = -99, nones = 0;
        with_kind(kind, [&](auto K) { ++calls; seen = decltype(K)::value; }, [&] { ++nones; });
        CHECK(calls == 1 && seen == kind && nones == 0);
    }
    for (int kind : {-1, 6}) {
        int calls = 0, nones = 0;
        with_kind(kind, [&](auto) { ++calls; }, [&] { ++nones; });
        CHECK(calls == 0 && nones == 1);
    }
    return 0;
}

int main()
{
    if (test_layouts() || test_split() || test_views() || test_event_pairs() || test_with_kind()) return 1;
    for (void* p : g_freed) std::free(p);
    std::printf("QUERY_HOST_OK\n");
    return 0;
}
