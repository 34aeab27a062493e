// stage_layout.h -- internal: how the query entries (abi_quote.cpp, abi_swap.cpp, abi_quote_path.cpp, abi_swap_path.cpp for
// itself and abi_swap_order.cpp, abi_find_path.cpp (both find entries and cfmm_find_disjoint_paths), abi_size_path.cpp,
// abi_split_paths.cpp) carve their ONE pinned staging buffer of 8-byte words into typed columns.  No HIP, no context.
// A layout is declared once, column by column; each column starts on a word and takes ceil(bytes / 8) words.  The entry grows
// its buffer by words() and takes every host pointer from the column's handle, so the size and the addresses cannot disagree.
// What crosses to the device in ONE copy is ONE column (the [2][count] coins, n_hops with the three int32 hop columns, ...).
#pragma once

#include <cstddef>
#include <cstdint>

namespace cfmm {

constexpr size_t words_of(size_t bytes) { return (bytes + 7) / 8; }

template <class T>
struct StageCol {
    size_t off = 0, n = 0;   // first word, elements
    T* in(unsigned long long* stage) const { return reinterpret_cast<T*>(stage + off); }
};

class StageLayout {
    size_t words_ = 0;

public:
    template <class T>
    StageCol<T> add(size_t n)
    {
        const StageCol<T> col{words_, n};
        words_ += words_of(n * sizeof(T));
        return col;
    }
    size_t words() const { return words_; }
};

// The entries' layouts for n queries / paths of at most H hops (nh = n * H).  Members are initialised in the order they are
// declared, which is the order of the columns.  `table_bytes`: the entry's segment table (seg_view.h), first.
struct QuoteStage {   // cfmm_quote / cfmm_quote_out
    StageLayout l;
    StageCol<double> amt;
    StageCol<int32_t> coins;    // [2][n] coin_in, coin_out
    StageCol<double> out;
    StageCol<long long> idx;    // only where the call has one
    QuoteStage(size_t n, bool has_idx) : amt(l.add<double>(n)), coins(l.add<int32_t>(2 * n)), out(l.add<double>(n)), idx(l.add<long long>(has_idx ? n : 0)) {}
};
struct RateStage {   // cfmm_quote_rate: QuoteStage's columns (amt: only where the call has amounts) and the rates
    StageLayout l;
    StageCol<double> amt;
    StageCol<int32_t> coins;    // [2][n] coin_in, coin_out
    StageCol<double> out;       // [2][n] amount_out, rate
    StageCol<long long> idx;    // only where the call has one
    RateStage(size_t n, bool has_amt, bool has_idx)
        : amt(l.add<double>(has_amt ? n : 0)), coins(l.add<int32_t>(2 * n)), out(l.add<double>(2 * n)), idx(l.add<long long>(has_idx ? n : 0)) {}
};
struct SwapStage {   // cfmm_swap / cfmm_swap_out / cfmm_swap_limit, the swaps in wave order; price: UniV3 segments, limit / status: cfmm_swap_out and cfmm_swap_limit
    StageLayout l;
    StageCol<double> amt;
    StageCol<int32_t> coins;    // [2][n]
    StageCol<double> out, price;
    StageCol<long long> idx;
    StageCol<double> limit;
    StageCol<int32_t> status;
    StageCol<int> left;         // [1] the window flag
    StageCol<double> used;      // cfmm_swap_limit: amount_used
    SwapStage(size_t n, bool has_idx, bool univ3, bool has_limit, bool has_status, bool has_used = false)
        : amt(l.add<double>(n)), coins(l.add<int32_t>(2 * n)), out(l.add<double>(n)), price(l.add<double>(univ3 ? n : 0)),
          idx(l.add<long long>(has_idx ? n : 0)), limit(l.add<double>(has_limit ? n : 0)), status(l.add<int32_t>(has_status ? n : 0)),
          left(l.add<int>(1)), used(l.add<double>(has_used ? n : 0)) {}
};
struct PathStage {   // cfmm_quote_path / cfmm_quote_path_out (the _dev entries: the table alone, n = 0)
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> i32;      // [1 + 3*H][n] n_hops, hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [H][n]
    StageCol<double> given, answer, hops;   // hops: [H][n], only where the call wants them
    PathStage(size_t table_bytes, size_t n, size_t nh, bool want_hops)
        : table(l.add<unsigned char>(table_bytes)), i32(l.add<int32_t>(n + 3 * nh)), row(l.add<long long>(nh)), given(l.add<double>(n)),
          answer(l.add<double>(n)), hops(l.add<double>(want_hops ? nh : 0)) {}
};
struct PathRateStage {   // cfmm_quote_path_rate (cfmm_quote_path_rate_dev: the table alone, n = 0)
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> i32;      // [1 + 3*H][n] n_hops, hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [H][n]
    StageCol<double> given;
    StageCol<double> answer;    // [2][n] amount_out, rate
    StageCol<double> hops;      // [2][H][n] hop_out, hop_rate (the half the call does not want: unused)
    PathRateStage(size_t table_bytes, size_t n, size_t nh)
        : table(l.add<unsigned char>(table_bytes)), i32(l.add<int32_t>(n + 3 * nh)), row(l.add<long long>(nh)), given(l.add<double>(n)),
          answer(l.add<double>(2 * n)), hops(l.add<double>(2 * nh)) {}
};
struct SizeStage {   // cfmm_size_path (cfmm_size_path_dev: the table alone, n = 0)
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> i32;      // [1 + 3*H][n] n_hops, hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [H][n]
    StageCol<double> in;        // [3][n] max_amount_in, value_in, value_out (a value the call does not give: unused)
    StageCol<double> out;       // [3][n] amount_in, amount_out, gain
    StageCol<int32_t> status;   // [n]
    SizeStage(size_t table_bytes, size_t n, size_t nh)
        : table(l.add<unsigned char>(table_bytes)), i32(l.add<int32_t>(n + 3 * nh)), row(l.add<long long>(nh)), in(l.add<double>(3 * n)),
          out(l.add<double>(3 * n)), status(l.add<int32_t>(n)) {}
};
struct SplitStage {   // cfmm_split_paths: g orders over n paths (cfmm_split_paths_dev: the table alone, g = n = 0)
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> i32;      // [1 + 3*H][n] n_hops, hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [H][n] hop_row, then [g + 1] order_first
    StageCol<double> amount;    // [g]
    StageCol<double> out;       // [2][n] path_amount_in, path_amount_out, then [g] total_out
    StageCol<int32_t> status;   // [g]
    SplitStage(size_t table_bytes, size_t g, size_t n, size_t nh)
        : table(l.add<unsigned char>(table_bytes)), i32(l.add<int32_t>(n + 3 * nh)), row(l.add<long long>(nh + (g ? g + 1 : 0))),
          amount(l.add<double>(g)), out(l.add<double>(2 * n + g)), status(l.add<int32_t>(g)) {}
};
struct SwapPathStage {   // cfmm_swap_path(_out) and cfmm_swap_order(_out): g orders (the path entries: 0) over n paths, in wave
                         // order; nrec: the table's records, one window flag each
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> i32;      // [1 + 3*H][n]
    StageCol<long long> row;    // [H][n] hop_row, then [g + 1] order_first
    StageCol<double> amt;       // [n] the given amounts, then the limits: [g], the path entries [n]
    StageCol<double> out;       // [n] the paths' answers, then [g] the totals
    StageCol<double> hops, price;
    StageCol<int32_t> status;   // [n] the paths' statuses, then [g] the orders'
    StageCol<int> left;         // [nrec]
    SwapPathStage(size_t table_bytes, size_t nrec, size_t n, size_t nh, size_t g = 0)
        : table(l.add<unsigned char>(table_bytes)), i32(l.add<int32_t>(n + 3 * nh)), row(l.add<long long>(nh + (g ? g + 1 : 0))),
          amt(l.add<double>(n + (g ? g : n))), out(l.add<double>(n + g)), hops(l.add<double>(nh)), price(l.add<double>(nh)),
          status(l.add<int32_t>(n + g)), left(l.add<int>(nrec)) {}
};
struct FindStage {   // cfmm_find_path / cfmm_find_path_out
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> tok;      // [2][n] token_in, token_out
    StageCol<double> amt, out;
    StageCol<int32_t> ns;       // [2][n] n_hops, status
    StageCol<int32_t> hop32;    // [3][H][n] hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [H][n]
    FindStage(size_t table_bytes, size_t n, size_t nh)
        : table(l.add<unsigned char>(table_bytes)), tok(l.add<int32_t>(2 * n)), amt(l.add<double>(n)), out(l.add<double>(n)),
          ns(l.add<int32_t>(2 * n)), hop32(l.add<int32_t>(3 * nh)), row(l.add<long long>(nh)) {}
};
struct FindDisjointStage {   // cfmm_find_disjoint_paths: n queries, K paths each, nh = n * H
    StageLayout l;
    StageCol<unsigned char> table;
    StageCol<int32_t> tok;      // [2][n] token_in, token_out
    StageCol<double> amt;       // [n]
    StageCol<double> out;       // [K][n]
    StageCol<int32_t> ns;       // [n] n_paths, then [2][K][n] n_hops, status
    StageCol<int32_t> hop32;    // [3][K][H][n] hop_seg, hop_coin_in, hop_coin_out
    StageCol<long long> row;    // [K][H][n]
    FindDisjointStage(size_t table_bytes, size_t n, size_t K, size_t nh)
        : table(l.add<unsigned char>(table_bytes)), tok(l.add<int32_t>(2 * n)), amt(l.add<double>(n)), out(l.add<double>(K * n)),
          ns(l.add<int32_t>(n + 2 * K * n)), hop32(l.add<int32_t>(3 * K * nh)), row(l.add<long long>(K * nh)) {}
};

} // namespace cfmm
