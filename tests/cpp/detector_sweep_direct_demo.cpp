/* Two urf::Detectors over the same sequence of sweeps, road_marker, the reference order and setSweepOutputs on in both, the sweeps kept
 * URF_MAX_IN_FLIGHT in flight (submit(); once four are out, collect() the oldest):
 *   A  setSweepResultsDirect off: the sequence copies header and three lists of the sweep's length to the slot's pinned buffer;
 *   B  setSweepResultsDirect(true): the kernels store marker points, counts and the packed lists into the slot's mapped buffer.
 * Everything either publishes per sweep -- the four clouds as bytes, the MarkerArray with its DELETE ghosts (the marker builder keeps
 * state between sweeps: tickets are collected in submission order) -- is serialised and compared byte for byte.
 *   usage: detector_sweep_direct_demo cloud.bin [cloud.bin ...]     cloud.bin: u32 n, float x[n], y[n], z[n]
 *   prints: sweeps S equal E published P deletes D road R ; exit status 0 iff E == S
 * (links the product library only: the sweeps come from the test) */
#include <cstdio>
#include <cstring>
#include <deque>
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

/* every sweep through one detector, four in flight; false when the switch could be changed under them */
bool run(const std::vector<urf::PointCloud>& clouds, size_t n_max, bool direct, std::vector<std::string>& out, Tally& t)
{
    urf::Detector det(0, (uint32_t)n_max);
    if (direct)
        det.setSweepResultsDirect(true);   /* (before the bits: the setter that comes second allocates) */
    urf_params p = det.params();
    p.min_X = p.min_Y = -200.f;
    p.max_X = p.max_Y = 200.f;
    det.setParams(p);
    det.setSweepOutputs(true);
    det.enableRoadMarker(true);
    det.setReferenceOrder(true);
    std::deque<uint32_t> tickets;
    bool refused = true;
    for (const auto& c : clouds) {
        if (tickets.size() == URF_MAX_IN_FLIGHT) {
            out.push_back(published_by(det, det.collect(tickets.front()), t));
            tickets.pop_front();
        }
        tickets.push_back(det.submit(c));
        bool busy = false;   /* the switch cannot change under the sweeps in flight */
        try {
            det.setSweepResultsDirect(!direct);
        } catch (const urf::Error& e) {
            busy = e.code == URF_ERR_BUSY;
        }
        refused = refused && busy;
    }
    while (!tickets.empty()) {
        out.push_back(published_by(det, det.collect(tickets.front()), t));
        tickets.pop_front();
    }
    return refused;
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
        std::vector<std::string> a, b;
        Tally ta, tb;
        if (!run(clouds, n_max, false, a, ta) || !run(clouds, n_max, true, b, tb)) {
            std::fprintf(stderr, "setSweepResultsDirect with sweeps in flight was not refused\n");
            return 4;
        }
        size_t equal = 0;
        for (size_t k = 0; k < a.size(); k++)
            equal += a[k] == b[k];
        std::printf("sweeps %zu equal %zu published %u deletes %u road %zu\n", a.size(), equal, tb.published, tb.deletes, tb.road);
        return equal == a.size() && a.size() == b.size() && ta.published == tb.published && ta.road == tb.road ? 0 : 1;
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
}
