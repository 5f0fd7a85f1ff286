/* Two urf::Detectors over the same sequence of sweeps, road_marker and the reference order on in both:
 *   A  one filtered() per sweep, setSweepOutputs off: urf_marker_points / urf_ordered_indices after every wait;
 *   B  setSweepOutputs(true), submit() x URF_MAX_IN_FLIGHT, then collect(): marker points and index lists travel with the ticket.
 * Everything either publishes per sweep -- the four clouds as bytes, the MarkerArray with its DELETE ghosts (the marker builder keeps
 * state between sweeps: tickets are collected in submission order) -- is serialised and compared byte for byte.
 *   usage: detector_sweep_outputs_demo cloud.bin [cloud.bin ...]     cloud.bin: u32 n, float x[n], y[n], z[n]
 *   prints: sweeps S equal E published P deletes D road R ; exit status 0 iff E == S
 * (links the product library only: the sweeps come from the test) */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "detector.hpp"

namespace {

template <class T>
void put(std::string& s, const T& v)
{
    s.append((const char*)&v, sizeof(T));
}

void put_cloud(std::string& s, const urf::PointCloud& c)
{
    put(s, c.header.seq);
    put(s, (uint64_t)c.points.size());
    s.append((const char*)c.points.data(), c.points.size() * sizeof(urf::PointXYZI));
}

struct Tally {
    unsigned published = 0, deletes = 0;
    size_t road = 0;
};

std::string published_by(const urf::Detector& det, bool ok, Tally& t)
{
    std::string s;
    put(s, (uint32_t)ok);
    put_cloud(s, det.roi());
    put_cloud(s, det.road());
    put_cloud(s, det.curb());
    put_cloud(s, det.road_probably());
    t.road += det.road().points.size();
    const urf::MarkerArray* ma = det.road_marker();
    put(s, (uint32_t)(ma ? 1 : 0));
    if (!ma)
        return s;
    t.published++;
    put(s, (uint64_t)ma->markers.size());
    for (const urf::Marker& m : ma->markers) {
        t.deletes += m.action == urf::Marker::DELETE;
        put(s, m.id);
        put(s, m.action);
        put(s, m.type);
        s += m.frame_id;
        put(s, m.position);
        put(s, m.orientation);
        put(s, m.scale);
        put(s, m.color);
        put(s, (uint64_t)m.points.size());
        for (const auto& q : m.points)
            put(s, q);
    }
    return s;
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    std::vector<urf::PointCloud> clouds;
    size_t n_max = 0;
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
        n_max = n > n_max ? n : n_max;
        clouds.push_back(std::move(cloud));
    }
    try {
        auto prepare = [](urf::Detector& det) {
            urf_params p = det.params();
            p.min_X = p.min_Y = -200.f;
            p.max_X = p.max_Y = 200.f;
            det.setParams(p);
            det.enableRoadMarker(true);
            det.setReferenceOrder(true);
        };
        std::vector<std::string> a, b;
        Tally ta, tb;
        {
            urf::Detector det(0, (uint32_t)n_max);
            prepare(det);
            for (const auto& c : clouds)
                a.push_back(published_by(det, det.filtered(c), ta));
        }
        {
            urf::Detector det(0, (uint32_t)n_max);
            det.setSweepOutputs(true);   /* (before or after the two others: the bits follow all three) */
            prepare(det);
            for (size_t k0 = 0; k0 < clouds.size(); k0 += URF_MAX_IN_FLIGHT) {
                uint32_t tickets[URF_MAX_IN_FLIGHT];
                size_t m = 0;
                for (; m < URF_MAX_IN_FLIGHT && k0 + m < clouds.size(); m++)
                    tickets[m] = det.submit(clouds[k0 + m]);
                bool busy = false;   /* the switch cannot change under the sweeps in flight */
                try {
                    det.setSweepOutputs(false);
                } catch (const urf::Error& e) {
                    busy = e.code == URF_ERR_BUSY;
                }
                if (!busy) {
                    std::fprintf(stderr, "setSweepOutputs with sweeps in flight was not refused\n");
                    return 4;
                }
                for (size_t j = 0; j < m; j++)
                    b.push_back(published_by(det, det.collect(tickets[j]), tb));
            }
        }
        size_t equal = 0;
        for (size_t k = 0; k < a.size(); k++)
            equal += a[k] == b[k];
        std::printf("sweeps %zu equal %zu published %u deletes %u road %zu\n", a.size(), equal, tb.published, tb.deletes, tb.road);
        return equal == a.size() && ta.published == tb.published && ta.road == tb.road ? 0 : 1;
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
}
