// pair_forms_selftest.cpp -- the pair engine's form resolver, the generator of the listed forms and pwa_selftest_host as a stand-alone
// host program (no GPU is touched: kernel host stubs have addresses without a device), for a sanitizer run of that host code.
// From bioinformatics-algorithms_amd/csrc, after `make` (the other objects are linked as they are):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined -c -o /tmp/pwalign_ctx_san.o pwalign_ctx.hip
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -c -o /tmp/pair_forms_selftest.o ../../tools/pair_forms_selftest.cpp
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread -o /tmp/pair_forms_selftest /tmp/pair_forms_selftest.o \
//         /tmp/pwalign_ctx_san.o $(ls *.o | grep -v '^pwalign_ctx.o$')
//   /tmp/pair_forms_selftest
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "../include/pwalign.h"

int main() {
    uint32_t count = 0;
    if (pwa_pair_form_table(0xffffffffu, nullptr, &count) != PWA_E_INVALID || count == 0) return std::printf("listing: no count\n"), 1;
    std::set<std::string> names;
    for (uint32_t i = 0; i < count; ++i) {
        const char* name = nullptr;
        if (pwa_pair_form_table(i, &name, nullptr) != PWA_OK || !name || !*name) return std::printf("listing: entry %u\n", i), 1;
        names.insert(name);
    }
    if (names.size() != count) return std::printf("listing: %zu distinct names of %u\n", names.size(), count), 1;
    const char* past = nullptr;
    if (pwa_pair_form_table(count, &past, nullptr) != PWA_E_INVALID || past) return std::printf("listing: past the end\n"), 1;
    for (const uint32_t seed : {0u, 1u, 7u}) {
        const int rc = pwa_selftest_host(seed);
        if (rc) return std::printf("pwa_selftest_host(%u): check %d\n", seed, rc), 1;
    }
    std::printf("%u forms, pwa_selftest_host 0\n", count);
    return 0;
}
