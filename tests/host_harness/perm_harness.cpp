// TEST TOOL: compiles the product's permutation header (csrc/bg_perm.h) with g++ so that the mini-batch shuffle can be checked on a CPU-only machine
// and compared bit for bit with the device's bg_perm_fill.
#include "../../booster_gym_amd/csrc/bg_perm.h"
extern "C" void hh_perm_fill(unsigned n, unsigned long long seed, unsigned update, unsigned epoch, int* perm) {
    const bg::PermKey key{seed, update, epoch};
    for (unsigned i = 0; i < n; i++) perm[i] = (int)bg::perm_index(key, n, i);
}
extern "C" int hh_perm_half_bits(unsigned n) { return bg::perm_half_bits(n); }
