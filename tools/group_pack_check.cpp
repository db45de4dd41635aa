// The self-tests of a group call's host-only parts as a stand-alone host program, for a run under the host sanitizers (DESIGN.md
// "Many small LPs", group launches and group re-solve): the packing layout (group_pack.cpp) and the table builder (group_table.cpp).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ihpr-lp-c_amd/csrc tools/group_pack_check.cpp
//       hpr-lp-c_amd/csrc/group_pack.cpp hpr-lp-c_amd/csrc/group_table.cpp -o build/group_pack_check && build/group_pack_check
// (one command line.)
// Needs no GPU and no HIP.
#include <cstdio>

#include "group_pack.h"
#include "group_table.h"

int main() {
    const int pack = hprlp_group_pack_selftest();
    std::printf("group pack self-test: %s (%d)\n", pack == 0 ? "ok" : "FAILED at check", pack);
    const int table = hprlp_group_table_selftest();
    std::printf("group table self-test: %s (%d)\n", table == 0 ? "ok" : "FAILED at check", table);
    return pack == 0 && table == 0 ? 0 : 1;
}
