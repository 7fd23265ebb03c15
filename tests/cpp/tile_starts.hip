// tile_starts.hip -- prints the tile geometry of scan_kernel.h for the launches named on the command line, so that the
// Python mirror of it (tests/candidate_model.py) can be pinned against the header itself.  Built with hipcc and run on the
// CPU by tests/test_candidate_model_cpu.py.
//   tile_starts n_offsets passes big_tiles [...]  ->  one line per launch: tile_count, then tile_first_run of every tile
//   and of the one past the last, then tile_passes of every tile.
#include <cstdio>
#include <cstdlib>

#include "../../adsbdec_amd/csrc/scan_kernel.h"

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: tile_starts n_offsets passes big_tiles [...]\n");
        return 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
        const uint64_t n = strtoull(argv[a], nullptr, 10);
        const int k = atoi(argv[a + 1]);
        const uint32_t big = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
        const uint32_t tiles = adsb::tile_count(n, big, k);
        printf("%u", tiles);
        for (uint32_t t = 0; t <= tiles; t++)
            printf(" %llu", (unsigned long long)adsb::tile_first_run(t, big, k));
        for (uint32_t t = 0; t < tiles; t++)
            printf(" %d", adsb::tile_passes(t, big, k));
        printf("\n");
    }
    return 0;
}
