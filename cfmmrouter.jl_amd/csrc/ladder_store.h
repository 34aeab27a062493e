// ladder_store.h -- internal, host only: the tick ladders of one UniV3 segment as the host keeps them (Segment::lad), in a form
// that lets ONE pool's ladder change length without moving the others (cfmm_pools_set_ticks, abi_update.cpp).
//
// Representation: per pool a begin and a length over two arenas.  `base` holds the ladders as uploaded, in pool order; a
// ladder that no longer fits its slot is appended to `ext`, and what it leaves behind is garbage.  A replacement costs
// O(its own ticks); no other pool's ticks move.  Garbage is bounded: once it exceeds half of the live ticks (+ 4096) the
// next replacement re-tightens -- one O(T) pass that lays every ladder back into `base` in pool order -- so the arenas never
// hold more than 1.5 T + 4096 ticks, and the pass is paid once per T/2 replaced ticks (amortised O(1) per tick replaced).
// csr() hands out the tight CSR form (univ3_build's input; cfmm_update_reserves), re-tightening first when needed.
// No HIP call, no context: tests/native/ladder_store_host.cpp drives it on the CPU under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace cfmm {

class LadderStore {
    std::vector<double> lt_, liq_;     // base arena
    std::vector<double> xlt_, xliq_;   // ext arena: ladders that outgrew their slot
    std::vector<int64_t> beg_;         // >= 0: offset in base; < 0: offset −(beg + 1) in ext
    std::vector<int64_t> len_;
    std::vector<int64_t> off_;         // [m + 1] CSR offsets over base, valid while tight_
    int64_t live_ = 0;                 // Σ len
    bool tight_ = true;                // base holds exactly the live ticks, in pool order, and ext is empty

    int64_t held() const { return (int64_t)lt_.size() + (int64_t)xlt_.size(); }

public:
    // m ladders in CSR form (tick_off[0] == 0, non-decreasing: the upload has checked them)
    void assign(int64_t m, const int64_t* tick_off, const double* lower_ticks, const double* liquidity)
    {
        const int64_t T = m > 0 ? tick_off[m] : 0;
        lt_.assign(lower_ticks, lower_ticks + T);
        liq_.assign(liquidity, liquidity + T);
        xlt_.clear();
        xliq_.clear();
        off_.assign(tick_off, tick_off + (m > 0 ? m + 1 : 0));
        if (m == 0) off_.assign(1, 0);
        beg_.assign(off_.begin(), off_.end() - 1);
        len_.resize((size_t)m);
        for (int64_t i = 0; i < m; ++i) len_[(size_t)i] = tick_off[i + 1] - tick_off[i];
        live_ = T;
        tight_ = true;
    }

    int64_t pools() const { return (int64_t)len_.size(); }
    int64_t ticks_total() const { return live_; }          // Segment::n_ticks_total
    int64_t ticks_held() const { return held(); }          // live + garbage
    int64_t count(int64_t i) const { return len_[(size_t)i]; }
    const double* lower_ticks(int64_t i) const
    {
        const int64_t b = beg_[(size_t)i];
        return b >= 0 ? lt_.data() + b : xlt_.data() + (-b - 1);
    }
    const double* liquidity(int64_t i) const
    {
        const int64_t b = beg_[(size_t)i];
        return b >= 0 ? liq_.data() + b : xliq_.data() + (-b - 1);
    }

    // pool i's ladder becomes the nt >= 1 ticks lt / lq (which must not point into this store)
    void replace(int64_t i, int64_t nt, const double* lt, const double* lq)
    {
        const int64_t old = len_[(size_t)i];
        if (nt <= old) {   // into its own slot; a shorter ladder leaves the slot's end as garbage
            const int64_t b = beg_[(size_t)i];
            std::copy(lt, lt + nt, b >= 0 ? lt_.begin() + b : xlt_.begin() + (-b - 1));
            std::copy(lq, lq + nt, b >= 0 ? liq_.begin() + b : xliq_.begin() + (-b - 1));
            if (nt < old) tight_ = false;
        } else {
            beg_[(size_t)i] = -((int64_t)xlt_.size() + 1);
            xlt_.insert(xlt_.end(), lt, lt + nt);
            xliq_.insert(xliq_.end(), lq, lq + nt);
            tight_ = false;
        }
        len_[(size_t)i] = nt;
        live_ += nt - old;
        if (held() - live_ > live_ / 2 + 4096) tighten();
    }

    // every ladder back into base, in pool order, nothing else held
    void tighten()
    {
        if (tight_) return;
        std::vector<double> lt, liq;
        lt.reserve((size_t)live_);
        liq.reserve((size_t)live_);
        const int64_t m = pools();
        off_.resize((size_t)m + 1);
        for (int64_t i = 0; i < m; ++i) {
            const double *a = lower_ticks(i), *b = liquidity(i);
            const int64_t n = len_[(size_t)i];
            off_[(size_t)i] = (int64_t)lt.size();
            lt.insert(lt.end(), a, a + n);
            liq.insert(liq.end(), b, b + n);
        }
        off_[(size_t)m] = (int64_t)lt.size();
        std::copy(off_.begin(), off_.end() - 1, beg_.begin());
        lt_.swap(lt);
        liq_.swap(liq);
        std::vector<double>().swap(xlt_);
        std::vector<double>().swap(xliq_);
        tight_ = true;
    }

    // The CSR form of all ladders (valid until the next replace)
    struct Csr {
        const int64_t* tick_off;
        const double* lower_ticks;
        const double* liquidity;
    };
    Csr csr()
    {
        tighten();
        return Csr{off_.data(), lt_.data(), liq_.data()};
    }
};

} // namespace cfmm
