/*
 * policy_switch_walk.cpp -- what urf_policy::plan (urban_road_filter_amd/csrc/urf_policy.hpp, no HIP) makes of a batch call in front mode 3
 * at 64 lasers with the star-shaped search on, for the steps given on the command line as triples multi_sector multi_sector_cp curbPoints:
 * prints "front front_ms" per step.   g++ -std=c++17 -O2 -I include -I urban_road_filter_amd/csrc
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "urf_policy.hpp"

int main(int argc, char** argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        urf_policy p;
        p.front_mode = 3;
        p.multi_sector = atoi(argv[i]) != 0;
        p.multi_sector_cp = atoi(argv[i + 1]) != 0;
        urf_dev_params dp;
        memset(&dp, 0, sizeof dp);
        dp.p.channels = 64, dp.p.curbPoints = atoi(argv[i + 2]), dp.p.star_shaped_method = 1;
        urf_kargs a;
        memset(&a, 0, sizeof a);
        a.tiles = 8u, a.n_scans = 3u, a.capture = 0u;
        p.plan(a, dp, false, false);
        printf("%u %u\n", a.front, a.front_ms);
    }
    return 0;
}
