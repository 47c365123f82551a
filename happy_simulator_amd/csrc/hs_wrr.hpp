// hs_wrr.hpp -- host side of the table-driven load-balancing strategies (components/load_balancer/strategies.py):
//   * WeightedRoundRobin.select (:111-134), the smooth (nginx) algorithm, as ONE period of its selection sequence;
//   * IPHash.select (:320-333): int(md5(key).hexdigest(), 16) % len(backends).
// Shared by the load-balancer pipeline (hs_lb.hip) and the general-graph engine (hs_graph.hip); exact integer arithmetic throughout.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hs_ring.hpp"

namespace hs {
namespace wrr {

// Largest total weight whose table the engines build: 2^24 entries of int32 (64 MB on the device).  Beyond it the strategy is
// refused by name (HS_E_UNSUPPORTED), never truncated.
constexpr int64_t kMaxTotalWeight = 1ll << 24;

// One period of WeightedRoundRobin.select over backends 0 .. n-1 with weights w (all >= 1): out[k] = the backend of selection k,
// k in [0, W), W = sum(w); selection k of a run is out[k % W] (every current weight is back at 0 after W selections).
//
// The reference adds w_i to every current weight, takes the FIRST maximum and subtracts W from it: O(B) per selection.  Backends
// of equal weight are interchangeable up to their order, so the same sequence comes out of a per-class model in O(classes):
// a class of K members of weight w that has been chosen n times so far offers members[n % K] (the first of its members with
// the fewest selections) with current weight w * t - W * (n / K) at the 1-based step t; the largest offer wins, equal offers go
// to the smaller backend index (max() keeps the first maximum in add_backend order).  Returns W, or -1 for a weight < 1.
inline int64_t build_table(const int32_t *w, int n, std::vector<int32_t> &out) {
    out.clear();
    int64_t W = 0;
    for (int i = 0; i < n; ++i) {
        if (w[i] < 1) return -1;
        W += w[i];
    }
    struct Cls { int64_t w; std::vector<int32_t> members; int64_t turn, rounds; };
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return w[x] < w[y]; });
    std::vector<Cls> cls;
    for (int32_t i : order) {                          // (members stay in backend order: the sort is stable)
        if (cls.empty() || cls.back().w != w[i]) cls.push_back(Cls{w[i], {}, 0, 0});
        cls.back().members.push_back(i);
    }
    out.resize((size_t)W);
    for (int64_t t = 1; t <= W; ++t) {
        int best = -1; int64_t best_cw = 0; int32_t best_m = 0;
        for (int k = 0; k < (int)cls.size(); ++k) {
            const Cls &c = cls[(size_t)k];
            const int64_t cw = c.w * t - W * c.rounds;
            const int32_t m = c.members[(size_t)c.turn];
            if (best < 0 || cw > best_cw || (cw == best_cw && m < best_m)) { best = k; best_cw = cw; best_m = m; }
        }
        Cls &c = cls[(size_t)best];
        if (++c.turn == (int64_t)c.members.size()) { c.turn = 0; c.rounds += 1; }
        out[(size_t)(t - 1)] = best_m;
    }
    return W;
}

// IPHash.select for a key string: the 128-bit digest read as one big-endian integer, modulo the backend count
inline int32_t ip_hash_select(const char *key, size_t len, int32_t n_backends) {
    uint8_t dg[16];
    hs::ring::Md5 m;
    m.digest(key, len, dg);
    uint64_t r = 0;
    for (int i = 0; i < 16; ++i) r = ((r << 8) | dg[i]) % (uint64_t)n_backends;    // (r < 2^31: no overflow)
    return (int32_t)r;
}

}  // namespace wrr
}  // namespace hs
