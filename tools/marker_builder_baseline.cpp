/* The host baseline of tools/marker_strips_bench.py: what a checkout WITHOUT urf_marker_strips_batch offers for the line strips of a
 * batch -- urf::MarkerBuilder::build per sweep, one thread, on marker points already copied to the host.  Uses nothing but
 * urf::MarkerBuilder (marker.hpp) so that it compiles against, and links to, the parent commit's library.
 *   usage: marker_builder_baseline points.bin repeats      points.bin: u32 S, u32 count[S], float pts[S][361][4]
 *   prints: one JSON line { "scans", "markers", "points", "ms": [one figure per repeat] } */
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "marker.hpp"

int main(int argc, char** argv)
{
    if (argc < 3)
        return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t S = 0;
    if (!f || std::fread(&S, 4, 1, f) != 1)
        return 3;
    std::vector<uint32_t> cnt(S);
    std::vector<float> pts((size_t)S * 361 * 4);
    if (std::fread(cnt.data(), 4, S, f) != S || std::fread(pts.data(), 4, pts.size(), f) != pts.size())
        return 3;
    std::fclose(f);
    const int repeats = atoi(argv[2]);
    size_t markers = 0, points = 0;
    std::printf("{\"scans\": %u, \"ms\": [", S);
    for (int r = 0; r < repeats; r++) {
        urf::MarkerBuilder mb;   /* a drive from its start */
        urf::MarkerArray out;
        markers = points = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t s = 0; s < S; s++)
            if (mb.build(pts.data() + (size_t)s * 361 * 4, cnt[s], out)) {
                markers += out.markers.size();
                for (const auto& m : out.markers)
                    points += m.points.size();
            }
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%s%.4f", r ? ", " : "", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::printf("], \"markers\": %zu, \"points\": %zu}\n", markers, points);
    return 0;
}
