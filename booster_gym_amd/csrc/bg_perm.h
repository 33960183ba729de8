// Keyed permutation of [0, n) evaluated per index (runner.num_mini_batches: the shuffle of a PPO mini-epoch's rows).  Stateless: no sort, no
// table, no generator state -- perm_index(key, n, i) is a bijection of [0, n) for every key, so a kernel fills pi with one thread per index and
// a host harness (tests/host_harness/perm_harness.cpp) computes the same numbers with g++.
//
//   * a balanced Feistel network on 2h bits, 2h = ceil(log2 n) rounded up to an even number (at least 2): (L, R) -> (R, L ^ F_r(R)), PERM_ROUNDS
//     rounds.  A Feistel network is a bijection of [0, 2^2h) whatever F is;
//   * F_r(R) = the low h bits of the first word of philox4x32_10 (bg_rng.h) on key (seed) and counter (R, round | mini-epoch << 8, RS_PERM,
//     update counter): a different function for every round, mini-epoch, update and seed (the rank enters through the seed, as in the rollout's
//     action noise);
//   * cycle walking: an image at or beyond n is encrypted again until it falls below n.  The walk follows the cycle of the 2^2h-permutation
//     that contains i, so it returns below n after at most 2^2h - n + 1 steps and the restriction to [0, n) is again a bijection; 2^2h < 4 n, so
//     the expected number of steps is below 4.
//
// Six rounds: four give a pseudo-random permutation from pseudo-random round functions (Luby and Rackoff, SIAM J. Comput. 17(2), 1988) up to
// ~2^(h/2) queries, which a mini-epoch's n = 2^2h evaluations exceed, so two more rounds are run as margin (a fill of 98,304 indices takes 48 us on
// an MI355X, a chain of dependent multiplies rather than throughput: DESIGN.md section 6.9).
#pragma once
#include "bg_rng.h"

namespace bg {

constexpr int PERM_ROUNDS = 6;

struct PermKey {
    uint64_t seed;     // basic.seed with the rank folded in (utils/runner.py)
    uint32_t update;   // the runner's update counter
    uint32_t epoch;    // the mini-epoch inside the update (below 2^24)
};

// half the bit width of the Feistel domain: the smallest h >= 1 with 2^(2h) >= n
BG_HD int perm_half_bits(uint32_t n) {
    int h = 1;
    while (h < 16 && (1ull << (2 * h)) < (uint64_t)n) h++;
    return h;
}

BG_HD uint32_t perm_feistel(const PermKey& key, int h, uint32_t x) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t L = x >> h, R = x & mask;
    for (int r = 0; r < PERM_ROUNDS; r++) {
        uint32_t o[4];
        philox4x32_10((uint32_t)key.seed, (uint32_t)(key.seed >> 32), R, (uint32_t)r | (key.epoch << 8), (uint32_t)RS_PERM, key.update, o);
        const uint32_t t = L ^ (o[0] & mask);
        L = R;
        R = t;
    }
    return (L << h) | R;
}

// pi(i) for i < n, 1 <= n <= 2^31
BG_HD uint32_t perm_index(const PermKey& key, uint32_t n, uint32_t i) {
    const int h = perm_half_bits(n);
    uint32_t x = perm_feistel(key, h, i);
    while (x >= n) x = perm_feistel(key, h, x);
    return x;
}

}  // namespace bg
