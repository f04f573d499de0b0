// Which plan the probe build's dispatch makes for one uniform batch under the current
// environment: storm_amd/csrc/dispatch.h alone (no HIP, no library), compiled with
// -DSTORMCK_PROBES so that knobs() reads the same STORMCK_* variables as
// tools/libstormck_probes.so. tests/test_stream_kernels_gpu.py runs it under its child's
// environment to show, not assume, that a batch takes k_xxh64_glds_skew.
//   plan_query n len stride base_low4 ncu [verify]  ->  "<kernel> <grid> <block>"
#include "../../storm_amd/csrc/dispatch.h"

#include <cstdio>
#include <cstdlib>

#ifndef STORMCK_PROBES
#error "plan_query answers for the probe build: compile with -DSTORMCK_PROBES"
#endif

using namespace stormck;

static const char* name_of(Kernel k) {
    static const char* names[] = {"wide", "wide-multi", "glds-var", "glds-var-ordered", "glds", "glds-skew",
                                  "quad-spread", "quad", "pointer-pc", "too-large"};
    return names[static_cast<int>(k)];
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s n len stride base_low4 ncu [verify]\n", argv[0]);
        return 2;
    }
    Query q;
    q.n = std::strtoull(argv[1], nullptr, 10);
    q.len = static_cast<uint32_t>(std::strtoull(argv[2], nullptr, 10));
    q.stride = std::strtoull(argv[3], nullptr, 10);
    q.base_low4 = static_cast<unsigned>(std::strtoul(argv[4], nullptr, 10)) & 15u;
    const uint64_t ncu = std::strtoull(argv[5], nullptr, 10);
    q.verify = argc > 6 && std::atoi(argv[6]) != 0;
    const Plan p = plan_checksum(q, ncu, knobs());
    std::printf("%s %u %u\n", name_of(p.kernel), p.grid, p.block);
    return 0;
}
