// The packing layout's self-test as a stand-alone host program, for a run under the host sanitizers (DESIGN.md "Many small LPs",
// group re-solve):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ihpr-lp-c_amd/csrc \
//       tools/group_pack_check.cpp hpr-lp-c_amd/csrc/group_pack.cpp -o build/group_pack_check && build/group_pack_check
// Needs no GPU and no HIP.
#include <cstdio>

#include "group_pack.h"

int main() {
    const int failed = hprlp_group_pack_selftest();
    std::printf("group pack self-test: %s (%d)\n", failed == 0 ? "ok" : "FAILED at check", failed);
    return failed == 0 ? 0 : 1;
}
