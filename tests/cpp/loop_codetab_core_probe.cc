// Stand-alone probe of addapt_amd/csrc/loop_codetab_core.hpp (tests/test_loop_codetab_core.py).
//   probe build        the three source tables filled with values that differ in every
//                      entry (entry n of int11 | int21 | int22 laid end to end holds n in
//                      both halves); writes E (LCT_ALLOC uint16) to stdout
//   probe uneven K N   the same with the halves of entry N of table K (0 int11, 1 int21,
//                      2 int22) made unequal; prints loop_codetab_build's result
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "loop_codetab_core.hpp"

int main(int argc, char **argv) {
    using namespace adx;
    constexpr size_t N11 = 8 * 8 * 5 * 5, N21 = N11 * 5, N22 = N21 * 5;
    static_assert(N11 + N21 + N22 < 65536, "distinct 16-bit values");
    std::vector<uint32_t> t11(N11), t21(N21), t22(N22);
    uint32_t n = 0;
    for (auto *t : {&t11, &t21, &t22})
        for (auto &w : *t) w = n | (n << 16), n++;
    std::vector<uint16_t> E(LCT_ALLOC, 0xABCDu);
    if (argc >= 2 && !std::strcmp(argv[1], "build")) {
        if (!loop_codetab_build(t11.data(), t21.data(), t22.data(), E.data())) return 2;
        return std::fwrite(E.data(), sizeof(uint16_t), E.size(), stdout) == E.size() ? 0 : 3;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "uneven")) {
        std::vector<uint32_t> *t[3] = {&t11, &t21, &t22};
        t[std::atoi(argv[2])]->at(size_t(std::atol(argv[3]))) ^= 0x10000u;
        std::printf("%d\n", loop_codetab_build(t11.data(), t21.data(), t22.data(), E.data()) ? 1 : 0);
        return 0;
    }
    return 1;
}
