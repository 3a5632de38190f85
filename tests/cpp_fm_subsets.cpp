// se2lam_amd/csrc/fm_subsets.h compiled by the host compiler (tests/test_loop_verify_abi.py): prints the 7-point samples
// fm_draw_subsets gives for the point counts on the command line, from a table of argv[1] raw values (the full table for
// 0), so that a short table exercises the continuation of the recurrence behind it.
// argv[3] != 0 takes every window through the serial scan, the path a draw otherwise only takes for a sample that does not
// end inside its window.
//   cpp_fm_subsets <table length or 0> <niters> <serial 0/1> <n>...   ->   one line per n: "n v v v ..." (niters * 7 values)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../se2lam_amd/csrc/fm_subsets.h"

int main(int argc, char** argv) {
    if (argc < 5) return 1;
    int len = std::atoi(argv[1]);
    if (len <= 0) len = se2gpu::kFmRawTable;
    const int niters = std::atoi(argv[2]);
    const bool serial = std::atoi(argv[3]) != 0;
    std::vector<uint32_t> table(len);
    const uint64_t state = se2gpu::fm_raw_fill(table.data(), len);
    for (int a = 4; a < argc; ++a) {
        const int n = std::atoi(argv[a]);
        std::vector<int> sub((size_t)niters * 7, -1);
        se2gpu::fm_draw_subsets(table.data(), len, state, n, niters, sub.data(), 0, serial);
        std::printf("%d", n);
        for (int v : sub) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
