/* Two urf::Detectors over the same messages of different lengths (a dense stream: every callback has its own number of points):
 *   A  setSweepQuantum off, one filtered() per message;
 *   B  setSweepQuantum(2048), submit() for all of them, then collect().
 * The four clouds either publishes per message are serialised and compared byte for byte; B's context must have captured no more
 * sequences than there are padded lengths per slot.
 *   usage: detector_sweep_quantum_demo cloud.bin [cloud.bin ...]     cloud.bin: u32 n, float x[n], y[n], z[n]   (at most URF_MAX_IN_FLIGHT)
 *   prints: messages M equal E road R curb C ; exit status 0 iff E == M
 * (links the product library only: the sweeps come from the test) */
#include <cstdio>
#include <string>
#include <vector>

#include "detector.hpp"

namespace {

void put_cloud(std::string& s, const urf::PointCloud& c)
{
    const uint64_t n = c.points.size();
    s.append((const char*)&c.header.seq, sizeof(c.header.seq));
    s.append((const char*)&n, sizeof(n));
    s.append((const char*)c.points.data(), c.points.size() * sizeof(urf::PointXYZI));
}

std::string published_by(const urf::Detector& det, bool ok, size_t& road, size_t& curb)
{
    std::string s(ok ? "1" : "0");
    put_cloud(s, det.roi());
    put_cloud(s, det.road());
    put_cloud(s, det.curb());
    put_cloud(s, det.road_probably());
    road += det.road().points.size();
    curb += det.curb().points.size();
    return s;
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2 || argc > 1 + URF_MAX_IN_FLIGHT)
        return 2;
    std::vector<urf::PointCloud> clouds;
    for (int k = 1; k < argc; k++) {
        FILE* fi = std::fopen(argv[k], "rb");
        uint32_t n = 0;
        if (!fi || std::fread(&n, 4, 1, fi) != 1)
            return 3;
        std::vector<float> x(n), y(n), z(n);
        if (std::fread(x.data(), 4, n, fi) != n || std::fread(y.data(), 4, n, fi) != n || std::fread(z.data(), 4, n, fi) != n)
            return 3;
        std::fclose(fi);
        urf::PointCloud cloud;
        cloud.header.seq = (uint32_t)k;
        cloud.points.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            cloud.points[i].x = x[i];
            cloud.points[i].y = y[i];
            cloud.points[i].z = z[i];
            cloud.points[i].intensity = (float)(i % 251);
        }
        clouds.push_back(std::move(cloud));
    }
    try {
        auto prepare = [](urf::Detector& det) {
            urf_params p = det.params();
            p.min_X = p.min_Y = -200.f;
            p.max_X = p.max_Y = 200.f;
            p.channels = 32;
            det.setParams(p);
        };
        std::vector<std::string> a, b;
        size_t road_a = 0, curb_a = 0, road_b = 0, curb_b = 0;
        {
            urf::Detector det(0, 8192);
            prepare(det);
            for (const auto& c : clouds)
                a.push_back(published_by(det, det.filtered(c), road_a, curb_a));
        }
        {
            urf::Detector det(0, 8192);
            prepare(det);
            bool refused = false;   /* not a multiple of a tile */
            try {
                det.setSweepQuantum(1000);
            } catch (const urf::Error& e) {
                refused = e.code == URF_ERR_INVALID_ARG;
            }
            if (!refused) {
                std::fprintf(stderr, "setSweepQuantum(1000) was not refused\n");
                return 4;
            }
            det.setSweepQuantum(2048);
            std::vector<uint32_t> tickets;
            for (const auto& c : clouds)
                tickets.push_back(det.submit(c));
            for (uint32_t t : tickets)
                b.push_back(published_by(det, det.collect(t), road_b, curb_b));
        }
        size_t equal = 0;
        for (size_t k = 0; k < a.size(); k++)
            equal += a[k] == b[k];
        std::printf("messages %zu equal %zu road %zu curb %zu\n", a.size(), equal, road_b, curb_b);
        return equal == a.size() && road_a == road_b && curb_a == curb_b ? 0 : 1;
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
}
